"""GPU: the reference's frame-to-frame query set inside the gated map passes -- vslam_build_map_pnp_inputs_requery_dev against its siblings (with
every keypoint a feature: vslam_feature_matching_dev's table and vslam_build_map_pnp_inputs_gated_dev's inputs on it, bit for bit), a host-driven
pass loop against the CPU restatement of tests/feature_query_ref.py (feature lists, tables, inputs, states, windows), the refusals, and
KeyframePipeline(f2f_queries="features") on rendered frames; f2f_queries="all" is the pipeline without the argument, bit for bit."""
import numpy as np
import pytest

import feature_query_ref as FQ
import gated_map_ref as GR
import kf_gate_ref as KR
from test_feature_query_ref import matched_tracks
from test_gpu_gated_map import _GDev, _replay
from test_gpu_pose_map import XYZ_TOL, _solve_host, _tables, _window_form

pytestmark = pytest.mark.gpu


class _QDev(_GDev):
    """test_gpu_gated_map._GDev with the descriptors on the device and the requery entry"""

    def __init__(self, pkg, tables, desc):
        super().__init__(pkg, tables)
        self.desc = self._up(desc, np.uint8)

    def match_all(self, ctx):
        """vslam_feature_matching_dev on every pair with every keypoint a query: (table, counts)"""
        torch, F, cap = self.torch, self.F, self.cap
        out = torch.zeros((F - 1, cap, 16), dtype=torch.uint8, device="cuda"); n = torch.zeros(F - 1, dtype=torch.int32, device="cuda")
        gap = torch.ones(F - 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.feature_matching_dev(self.desc.data_ptr(), cap * 32, self.keep["nk"].data_ptr(), self.desc.data_ptr() + cap * 32, cap * 32,
                                 self.keep["nk"].data_ptr() + 4, gap.data_ptr(), 1, F - 1, cap, out.data_ptr(), cap, n.data_ptr())
        ctx.sync()
        return out.cpu().numpy().reshape(F - 1, -1).view(self.pkg.DMATCH_DTYPE).reshape(F - 1, cap), n.cpu().numpy()

    def requery(self, ctx, G, index_prev, inl_prev, states, table_prev=None, bad=None):
        """one pass through vslam_build_map_pnp_inputs_requery_dev; table_prev = (f2f, nf2f) host arrays the walk reads (None: the tables' own); bad: arguments replaced (refusals)"""
        torch, F, cap = self.torch, self.F, self.cap
        tG, ts = self._up(G, np.float64), self._up(states, np.int32)
        t_idx = None if index_prev is None else self._up(index_prev, np.int32)
        t_inl = self.keep["inl"] if inl_prev is None else self._up(inl_prev, np.uint8)
        self.tr.d_pose_inlier = t_inl.data_ptr(); self.tr.pnp_capacity = cap if inl_prev is None else inl_prev.shape[1]
        if table_prev is not None:
            tf, tn = self._up(table_prev[0].view(np.uint8), np.uint8), self._up(table_prev[1], np.int32)
            self.tr.d_f2f = tf.data_ptr(); self.tr.d_nf2f = tn.data_ptr()
        o = dict(xyz=torch.full((F - 1, cap, 3), -5.0, dtype=torch.float32, device="cuda"), uv=torch.full((F - 1, cap, 2), -5.0, device="cuda"),
                 n=torch.full((F - 1,), -5, dtype=torch.int32, device="cuda"), index=torch.full((F - 1, cap), -5, dtype=torch.int32, device="cuda"),
                 st=torch.full((1,), -5, dtype=torch.int32, device="cuda"), feat=torch.full((F, cap), -5, dtype=torch.int32, device="cuda"),
                 nfeat=torch.full((F,), -5, dtype=torch.int32, device="cuda"), f2f=torch.zeros((F - 1, cap, 16), dtype=torch.uint8, device="cuda"),
                 nf2f=torch.full((F - 1,), -5, dtype=torch.int32, device="cuda"))
        a = dict(G=tG.data_ptr(), idx=None if t_idx is None else t_idx.data_ptr(), st=ts.data_ptr(), desc=self.desc.data_ptr(), stride=cap * 32,
                 feat=o["feat"].data_ptr(), nfeat=o["nfeat"].data_ptr(), f2f=o["f2f"].data_ptr(), nf2f=o["nf2f"].data_ptr())
        a.update(bad or {})
        torch.cuda.synchronize()
        try:
            ctx.build_map_pnp_inputs_requery_dev(self.tr, a["G"], a["idx"], a["st"], a["desc"], a["stride"], a["feat"], a["nfeat"], a["f2f"], a["nf2f"],
                                                 o["xyz"].data_ptr(), o["uv"].data_ptr(), o["n"].data_ptr(), o["index"].data_ptr(), cap, o["st"].data_ptr())
            ctx.sync()
        finally:
            self.tr.d_pose_inlier = self.keep["inl"].data_ptr(); self.tr.pnp_capacity = cap
            self.tr.d_f2f = self.keep["f2f"].data_ptr(); self.tr.d_nf2f = self.keep["nf2f"].data_ptr()
        r = {k: v.cpu().numpy() for k, v in o.items()}
        r["f2f"] = r["f2f"].reshape(F - 1, -1).view(self.pkg.DMATCH_DTYPE).reshape(F - 1, cap)
        return r


def _check_pass(dev, ref_pass, tag, n_feat=None):
    """a requery pass against the restatement's: feature lists, tables, counts, index maps and uv exact, positions within XYZ_TOL.  n_feat: the
    frames whose feature lists are compared (against the sequential loop the last frame's list is not final: it hangs on the last pair's links)"""
    F = len(dev["nfeat"])
    for f in range(F if n_feat is None else n_feat):
        want = ref_pass["feats"][f]
        assert dev["nfeat"][f] == len(want) and np.array_equal(dev["feat"][f, :len(want)], want), (tag, "feat", f)
    for i in range(F - 1):
        tab, it = ref_pass["tables"][i], ref_pass["items"][i]
        assert dev["nf2f"][i] == len(tab), (tag, "nf2f", i, dev["nf2f"][i], len(tab))
        for k in ("queryIdx", "trainIdx", "distance"):
            assert np.array_equal(dev["f2f"][k][i, :len(tab)], tab[k]), (tag, k, i)
        n = it["n"]
        assert dev["n"][i] == n == len(tab), (tag, i)
        assert np.array_equal(dev["index"][i, :n], np.arange(n)) and (dev["index"][i, n:] == -1).all(), (tag, "index", i)
        assert np.array_equal(dev["uv"][i, :n], it["uv"]), (tag, "uv", i)
        assert np.allclose(dev["xyz"][i, :n], it["xyz"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), (tag, "xyz", i)


@pytest.mark.parametrize("seed", range(2))
def test_every_keypoint_a_feature_is_the_gated_entry_on_the_unmasked_table(pkg, oracle, seed):
    """all keypoints depth-valid, all states 2: every keypoint is a feature whatever the links, so the feature lists are 0 .. n - 1, the table is
    vslam_feature_matching_dev's and the inputs are vslam_build_map_pnp_inputs_gated_dev's on that table, bit for bit"""
    rng = np.random.default_rng(6100 + seed)
    ctx = pkg.VO(device=0, max_batch=16)
    try:
        F = int(rng.integers(5, 10)); cap = int(rng.choice([128, 256]))
        t, desc = matched_tracks(rng, oracle, F, cap, valid_share=2.0)
        dv = _QDev(pkg, t, desc)
        table, ntab = dv.match_all(ctx)
        assert np.array_equal(ntab, t[7]) and all(np.array_equal(table[i, :ntab[i]], t[6][i, :ntab[i]]) for i in range(F - 1))   # (the oracle's)
        G0, st = dv.chain(ctx), np.full(F, 2, np.int32)
        a = dv.requery(ctx, G0, None, None, st)
        b = dv.inputs_gated(ctx, G0, None, None, st)
        assert a["st"][0] == 0 and np.array_equal(a["nf2f"], ntab) and (a["nfeat"] == cap).all() and (a["feat"] == np.arange(cap)[None, :]).all()
        for i in range(F - 1):
            assert a["f2f"][i, :ntab[i]].tobytes() == table[i, :ntab[i]].tobytes(), i
        for k in ("xyz", "uv", "n", "index", "st"):
            assert a[k].tobytes() == b[k].tobytes(), k
        # a second pass on map links: the index map and flags of the first
        G1, inl = _solve_host(a, G0, GR.gate_solver)
        a2 = dv.requery(ctx, G1, a["index"], inl, st, table_prev=(a["f2f"], a["nf2f"]))
        b2 = dv.inputs_gated(ctx, G1, a["index"], inl, st)
        for k in ("xyz", "uv", "n", "index", "st"):
            assert a2[k].tobytes() == b2[k].tobytes(), k
        assert a2["f2f"].tobytes() == a["f2f"].tobytes() and dv.requery(ctx, G1, a["index"], inl, st, table_prev=(a["f2f"], a["nf2f"]))["xyz"].tobytes() == a2["xyz"].tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(3))
def test_pass_loop_vs_restatement(pkg, oracle, seed):
    """passes 1 .. K on random tables and planted descriptors with the gate stand-in solver run on the host between them: every pass's feature lists,
    tables, inputs and states against the restatement's, the final windows against its windows; K = F - 1 also against the sequential loop"""
    rng = np.random.default_rng(6200 + seed)
    ctx = pkg.VO(device=0, max_batch=16, pnp_reproj_thr=(4.0, 300.0, 4.0)[seed])
    states, differ = set(), 0
    try:
        for case in range(2):
            F = int(rng.integers(6, 10)); cap = int(rng.choice([256, 384])); n_kf = int(rng.integers(2, 9)); policy = case % 2
            t, desc = matched_tracks(rng, oracle, F, cap, valid_share=rng.uniform(0.3, 0.9))
            match = FQ.oracle_matcher(oracle, desc, t[10])
            ninl0 = rng.integers(0, 200, F - 1)
            dv = _QDev(pkg, t, desc)
            G0 = dv.chain(ctx)
            st0 = dv.gate(ctx, t[9], 0, ninl0)
            seq = FQ.sequential(t, match, GR.gate_solver, n_kf=n_kf, policy=policy)
            for K in (1, 2, F - 1):
                tag = (seed, case, F, cap, K)
                ref = FQ.passes(t, match, GR.gate_solver, K, ninl0, G0=G0, n_kf=n_kf, policy=policy, reproj_thr=ctx.params.pnp_reproj_thr)
                assert np.array_equal(st0, ref["state0"]), tag
                G, index, inl, st, table = G0, None, None, st0, None
                for k in range(K):
                    d_in = dv.requery(ctx, G, index, inl, st, table_prev=table)
                    assert d_in["st"][0] == 0
                    _check_pass(d_in, ref["per_pass"][k], tag + (k,))
                    G, inl = _solve_host(d_in, G, GR.gate_solver)
                    index, table = d_in["index"], (d_in["f2f"], d_in["nf2f"])
                    st = dv.gate(ctx, G, 1, inl.sum(1))
                    assert np.array_equal(st, ref["per_pass"][k]["state"]), (tag, k)
                assert np.array_equal(G, ref["G"]), tag
                tf, tn = dv._up(table[0].view(np.uint8), np.uint8), dv._up(table[1], np.int32)
                dv.tr.d_f2f = tf.data_ptr(); dv.tr.d_nf2f = tn.data_ptr()
                w = dv.windows_gated(ctx, G, index, inl, st, n_kf=n_kf, policy=policy)
                dv.tr.d_f2f = dv.keep["f2f"].data_ptr(); dv.tr.d_nf2f = dv.keep["nf2f"].data_ptr()
                assert w["st"][0] == ref["status"] and np.array_equal(w["kf_frame"], ref["kf_frame"]) and np.array_equal(w["evicted"], ref["evicted"]), tag
                assert np.array_equal(w["nkf"], ref["n_kf"]), tag
                assert KR.same_windows(_window_form(w, F), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
                states |= set(st.tolist())
                if K == F - 1:
                    assert np.array_equal(G, seq["G"]) and np.array_equal(st, seq["state"]), tag
                    _check_pass(d_in, seq, tag + ("seq",), n_feat=F - 1)
                    for i in range(F - 1):
                        assert np.array_equal(inl[i, :seq["items"][i]["n"]], seq["items"][i]["mask"]), (tag, i)
                        differ += int(not np.array_equal(seq["tables"][i], t[6][i, :t[7][i]]))
                    assert KR.same_windows(_window_form(w, F), seq["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
        assert {1, 2} <= states and differ > 0, (states, differ)
    finally:
        ctx.close()


def test_refusals(pkg, oracle):
    rng = np.random.default_rng(6300)
    ctx = pkg.VO(device=0, max_batch=4)
    try:
        F, cap = 4, 128
        t, desc = matched_tracks(rng, oracle, F, cap, valid_share=0.7)
        dv = _QDev(pkg, t, desc)
        G0, st = dv.chain(ctx), np.full(F, 2, np.int32)
        dv.requery(ctx, G0, None, None, st)
        for bad in (dict(desc=None), dict(feat=None), dict(nfeat=None), dict(f2f=None), dict(nf2f=None), dict(st=None), dict(G=None),
                    dict(desc=dv.desc.data_ptr() + 8), dict(stride=cap * 32 + 8), dict(stride=cap * 16),
                    dict(f2f=dv.keep["f2f"].data_ptr()), dict(f2f=dv.keep["f2f"].data_ptr() + 16 * cap), dict(nf2f=dv.keep["nf2f"].data_ptr())):
            with pytest.raises(pkg.VslamError):
                dv.requery(ctx, G0, None, None, st, bad=bad)
        nk = dv.tr.d_nkps
        dv.tr.d_nkps = None
        with pytest.raises(pkg.VslamError):
            dv.requery(ctx, G0, None, None, st)
        dv.tr.d_nkps = nk
        dv.tr.d_T_abs = dv.keep["T"].data_ptr()
        with pytest.raises(pkg.VslamError):
            dv.requery(ctx, G0, None, None, st)
        dv.tr.d_T_abs = None
        small = pkg.VO(device=0, max_batch=2)   # three pairs do not fit a context of two
        try:
            with pytest.raises(pkg.VslamError):
                dv.requery(small, G0, None, None, st)
        finally:
            small.close()
        dv.requery(ctx, G0, None, None, st)
    finally:
        ctx.close()


def test_pipeline_feature_queries(pkg, oracle, synth):
    """16 rendered frames, RANSAC, f2f_queries="features", K = 1, 2 and 15, in the manner of test_gpu_gated_map.test_pipeline_per_pass_gate: the device's
    per-pass solver outputs replayed into the restatement reproduce its tables, feature lists, inputs, inlier counts and states exactly and its poses
    and windows within that test's tolerances; K = 15 is the sequential loop; the BA schedule runs on the windows; trajectory() gives the keyframes.
    Configuration: anms_num / seed were chosen on the restatement alone (oracle ORB, oracle matcher, oracle.pnp_ransac, no GPU) so that after frame 0
    it has frames of state 1 and of state 2, none of state 0, and feature-query tables that differ from stage A's.  Tried at seed 6: anms_num 500 --
    every frame a keyframe (at most 54 inliers), not used; 1000 -- states 2 1 2 1 2 2 1 2 2 2 1 2 1 2 1 2, all 15 tables differ, used; 1500 --
    states 2 1 1 2 1 2 1 2 1 2 1 2 1 2 1 2, would do as well."""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf, policy = 16, 10, 1
    seq = synth.stereo_sequence(B, seed=6)
    p = KeyframePipeline(B, anms_num=1000, n_kf=n_kf, unique_frames=B, seed=6, sequence=seq, ba_windows="tracks", pose="ransac", pose_inputs="map",
                         pose_passes=1, keyframe_gate="per_pass", window_policy="reference", f2f_queries="features")
    try:
        p.stage_orb(); p.stage_stereo_match()
        outs = {}
        for K in range(1, B):
            p.pose_passes = K
            p.stage_track()
            if K in (1, 2, B - 1):
                p.stage_build_windows()
            outs[K] = p.download()
        o1 = outs[1]
        t = _tables(o1, B)
        cap = o1["f2f"].shape[1]
        for K in range(2, B):   # stage A, its all-keypoint table included, is the same in every step
            for k in ("kps", "desc", "f2f", "nf2f", "inl", "Tpnp", "ninl"):
                assert np.array_equal(o1[k], outs[K][k]), (K, k)
        ninl0 = o1["ninl"][:B - 1]
        assert np.array_equal(o1["frame_state_prev"], GR.states0(t, ninl0))
        match = FQ.oracle_matcher(oracle, o1["desc"][:B], o1["cnt"][:B])
        solved = {K: (outs[K]["T_c_w"], outs[K]["map_inl"]) for K in outs}
        G0 = _QDev(pkg, t, o1["desc"][:B]).chain(p.vo)
        for i in (0, 5, B - 2):   # RANSAC against the oracle on a sample of pass 1's items
            n = int(o1["map_n"][i])
            wT, winl, wn, _ = oracle.pnp_ransac(o1["map_xyz"][i, :n], o1["map_uv"][i, :n])
            assert np.array_equal(o1["map_inl"][i, :n], winl) and o1["map_ninl"][i] == wn, i
            if wn > 0:
                assert np.allclose(o1["T_c_w"][i + 1], wT, rtol=1e-4, atol=1e-6), i
        for K in (1, 2, B - 1):
            o = outs[K]
            ref = FQ.passes(t, match, _replay(solved), K, ninl0, G0=G0, n_kf=n_kf, policy=policy)
            assert np.array_equal(ref["G"], o["T_c_w"]), K
            for k in range(K):
                assert np.array_equal(ref["per_pass"][k]["state"], outs[k + 1]["frame_state"]), (K, k)
                assert np.array_equal(ref["per_pass"][k]["num_inliers"], outs[k + 1]["map_ninl"][:B - 1]), (K, k)
            assert np.array_equal(ref["state"], o["frame_state"]), K
            dev = dict(feat=o["map_feat"], nfeat=o["map_nfeat"], f2f=o["map_f2f"][:B - 1], nf2f=o["map_nf2f"][:B - 1], n=o["map_n"], index=o["map_index"],
                       uv=o["map_uv"], xyz=o["map_xyz"])
            _check_pass(dev, ref["per_pass"][-1], K)
            g = dict(lm_off=o["ba_lm_off"], e_off=o["ba_e_off"], kf=o["ba_kf"], lm=o["ba_lm"], uv=o["ba_uv"], xyz=o["ba_xyz"], rel=o["ba_rel"])
            assert o["ba_build_status"][0] == ref["status"] and np.array_equal(o["ba_kf_frame"], ref["kf_frame"]), K
            assert np.array_equal(o["ba_evicted"], ref["evicted"]) and np.array_equal(o["ba_nkf"], ref["n_kf"]), K
            assert KR.same_windows(_window_form(g, B), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), K
        # K = F - 1: the sequential loop, whose solver outputs are the last pass's
        last = outs[B - 1]
        T15, inl15 = solved[B - 1]
        s = FQ.sequential(t, match, lambda i, xyz, uv, guess: (T15[i + 1], inl15[i, :len(uv)].astype(bool)), n_kf=n_kf, policy=policy)
        # what keeps this test from being vacuous, on the restatement's own result
        assert (s["state"][1:] == 1).any() and (s["state"][1:] == 2).any() and not (s["state"] == 0).any(), s["state"]
        assert any(not np.array_equal(s["tables"][i], o1["f2f"][i, :o1["nf2f"][i]]) for i in range(B - 1))
        assert np.array_equal(s["G"], last["T_c_w"]) and np.array_equal(s["state"], last["frame_state"])
        _check_pass(dict(feat=last["map_feat"], nfeat=last["map_nfeat"], f2f=last["map_f2f"][:B - 1], nf2f=last["map_nf2f"][:B - 1], n=last["map_n"],
                         index=last["map_index"], uv=last["map_uv"], xyz=last["map_xyz"]), s, "seq", n_feat=B - 1)
        for i in range(B - 1):
            assert np.array_equal(inl15[i, :s["items"][i]["n"]], s["items"][i]["mask"]), i
        g = dict(lm_off=last["ba_lm_off"], e_off=last["ba_e_off"], kf=last["ba_kf"], lm=last["ba_lm"], uv=last["ba_uv"], xyz=last["ba_xyz"],
                 rel=last["ba_rel"])
        assert KR.same_windows(_window_form(g, B), s["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1])
        # the BA schedule on the last windows; the trajectory: the keyframes
        p.vo.ba_batch_dev(p.ba_batch, schedule=1)
        kf = np.flatnonzero(last["frame_state"] == 2)
        assert (p.vo.ba_status(B)[kf] == 0).all()
        ids, T = p.trajectory()
        assert sorted(ids.tolist()) == kf.tolist()
        assert cap >= 1000
    finally:
        p.close()


def test_all_queries_is_the_pipeline_without_the_argument(synth):
    """f2f_queries="all" changes nothing: every downloaded array of a two-pass per_pass step equals the pipeline built without the argument"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = 16
    seq = synth.stereo_sequence(B, seed=6)
    kw = dict(anms_num=1000, n_kf=10, unique_frames=B, seed=6, sequence=seq, ba_windows="tracks", pose="ransac", pose_inputs="map", pose_passes=2,
              keyframe_gate="per_pass", window_policy="reference")
    a = KeyframePipeline(B, **kw); b = KeyframePipeline(B, f2f_queries="all", **kw)
    try:
        a.step(); b.step()
        oa, ob = a.download(), b.download()
        assert oa.keys() == ob.keys() and "map_f2f" not in ob
        for k in oa:
            assert np.array_equal(oa[k], ob[k]), k
    finally:
        a.close(); b.close()
