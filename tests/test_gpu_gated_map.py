"""The keyframe gate inside the map-based pose passes (keyframe_gate="per_pass"): vslam_gate_states_dev (kf_gate_kernel<true>),
vslam_build_map_pnp_inputs_gated_dev and vslam_build_windows_map_gated_dev against their ungated and stage-A siblings (the contracts of
include/vslam_hip.h, bit for bit), a host-driven pass loop against the CPU restatement of tests/gated_map_ref.py, and
KeyframePipeline(pose_inputs="map", keyframe_gate="per_pass") on rendered frames."""
import numpy as np
import pytest

import gated_map_ref as GR
import kf_gate_ref as KR
import pose_map_ref as PR
from test_gated_map_ref import dense_tracks
from test_gpu_kf_gate import _gate_inputs, _run_gated
from test_gpu_pose_map import XYZ_TOL, _check_items, _Dev, _solve_host, _tables, _window_form
from test_gpu_windows import _random_tracks

pytestmark = pytest.mark.gpu


def _outputs(pkg, F, n_kf, lm_cap, e_cap):
    """window outputs with the fill values of test_gpu_kf_gate._run_gated (an empty window leaves pose slots 1.. untouched) and their BaBatch"""
    import torch
    z = lambda n, dt, fill=0: torch.full(n if isinstance(n, tuple) else (n,), fill, dtype=dt, device="cuda")
    o = dict(lm_off=z(F + 1, torch.int32), e_off=z(F + 1, torch.int32), nkf=z(F, torch.int32, -5), T=z((F, n_kf, 7), torch.float64, -3.0),
             xyz=z((lm_cap, 3), torch.float32), rel=z(lm_cap, torch.uint8), inl=z(lm_cap, torch.uint8), kf=z(e_cap, torch.int32, -7),
             lm=z(e_cap, torch.int32), uv=z((e_cap, 2), torch.float32), st=z(1, torch.int32), kf_frame=z((F, n_kf), torch.int32, -9),
             evicted=z(F, torch.int32, -9))
    bb = pkg.BaBatch()
    bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["e_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
    bb.d_reliable = o["rel"].data_ptr(); bb.d_lm_inlier = o["inl"].data_ptr(); bb.d_kf_idx = o["kf"].data_ptr(); bb.d_lm_idx = o["lm"].data_ptr()
    bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["nkf"].data_ptr()
    return o, bb


class _GDev(_Dev):
    """test_gpu_pose_map._Dev with the gated entries"""

    def _up(self, a, dt):
        return self.torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()

    def gate(self, ctx, T, absolute, ninl):
        """vslam_gate_states_dev on host T (T_rel rows, or absolute G) and counts"""
        torch = self.torch
        tT, tn = self._up(T, np.float64), self._up(ninl, np.int32)
        st = torch.full((self.F,), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.gate_states_dev(self.F, tT.data_ptr(), absolute, tn.data_ptr(), st.data_ptr())
        ctx.sync()
        return st.cpu().numpy()

    def inputs_gated(self, ctx, G, index_prev, inl_prev, states, gated=True):
        """one pass through vslam_build_map_pnp_inputs_gated_dev (gated=False: the ungated entry, states ignored)"""
        torch, F, cap = self.torch, self.F, self.cap
        tG, ts = self._up(G, np.float64), self._up(states, np.int32)
        t_idx = None if index_prev is None else self._up(index_prev, np.int32)
        t_inl = self.keep["inl"] if inl_prev is None else self._up(inl_prev, np.uint8)
        self.tr.d_pose_inlier = t_inl.data_ptr(); self.tr.pnp_capacity = cap if inl_prev is None else inl_prev.shape[1]
        o = dict(xyz=torch.full((F - 1, cap, 3), -5.0, dtype=torch.float32, device="cuda"), uv=torch.full((F - 1, cap, 2), -5.0, device="cuda"),
                 n=torch.full((F - 1,), -5, dtype=torch.int32, device="cuda"), index=torch.full((F - 1, cap), -5, dtype=torch.int32, device="cuda"),
                 st=torch.full((1,), -5, dtype=torch.int32, device="cuda"))
        args = (o["xyz"].data_ptr(), o["uv"].data_ptr(), o["n"].data_ptr(), o["index"].data_ptr(), cap, o["st"].data_ptr())
        idx = None if t_idx is None else t_idx.data_ptr()
        torch.cuda.synchronize()
        if gated:
            ctx.build_map_pnp_inputs_gated_dev(self.tr, tG.data_ptr(), idx, ts.data_ptr(), *args)
        else:
            ctx.build_map_pnp_inputs_dev(self.tr, tG.data_ptr(), idx, *args)
        ctx.sync()
        self.tr.d_pose_inlier = self.keep["inl"].data_ptr(); self.tr.pnp_capacity = cap
        return {k: v.cpu().numpy() for k, v in o.items()}

    def windows_gated(self, ctx, G, index, inl, states, n_kf=10, policy=0, lm_cap=None, e_cap=None, gated=True):
        """vslam_build_windows_map_gated_dev (gated=False: vslam_build_windows_map_dev on the same outputs); every output back on the host"""
        torch, F, cap = self.torch, self.F, self.cap
        lm_cap = F * cap * (n_kf + 1) if lm_cap is None else lm_cap
        e_cap = 2 * F * cap * (n_kf + 1) if e_cap is None else e_cap
        tG, ts = self._up(G, np.float64), self._up(states, np.int32)
        t_idx = None if index is None else self._up(index, np.int32)
        t_inl = self.keep["inl"] if inl is None else self._up(inl, np.uint8)
        self.tr.d_pose_inlier = t_inl.data_ptr(); self.tr.pnp_capacity = cap if inl is None else inl.shape[1]
        o, bb = _outputs(self.pkg, F, n_kf, lm_cap, e_cap)
        idx = None if t_idx is None else t_idx.data_ptr()
        torch.cuda.synchronize()
        if gated:
            ctx.build_windows_map_gated_dev(self.tr, tG.data_ptr(), idx, ts.data_ptr(), n_kf, policy, 0.2, lm_cap, e_cap, bb, o["kf_frame"].data_ptr(),
                                            o["evicted"].data_ptr(), o["st"].data_ptr())
        else:
            ctx.build_windows_map_dev(self.tr, tG.data_ptr(), idx, n_kf, policy, 0.2, lm_cap, e_cap, bb, o["kf_frame"].data_ptr(), o["evicted"].data_ptr(),
                                      o["st"].data_ptr())
        ctx.sync()
        self.tr.d_pose_inlier = self.keep["inl"].data_ptr(); self.tr.pnp_capacity = cap
        return {k: v.cpu().numpy() for k, v in o.items()}


def _same(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        assert np.array_equal(a[k], b[k]), (tag, k)


# ------------------------------------------------------------------ 1. the contracts (a), (b), (c)
@pytest.mark.parametrize("seed", range(3))
def test_gate_states_contract(pkg, oracle, seed):
    """(c) absolute = 0 gives vslam_build_windows_gated_dev's d_frame_state bit for bit; absolute = 1 gives the restatement's gate on G_f o G_{f-1}^-1"""
    rng = np.random.default_rng(5100 + seed)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        seen = set()
        for case in range(4):
            F = int(rng.integers(2, 300)) if case == 3 else int(rng.integers(2, 40)); cap = 64; n_kf = int(rng.integers(1, 11))
            t = list(_random_tracks(rng, F, cap, cap))
            t[9], ninl = _gate_inputs(rng, F, oracle)
            t = tuple(t)
            want = _run_gated(pkg, ctx, t, ninl, n_kf, F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1), case % 2)["state"]
            dv = _GDev(pkg, t)
            assert np.array_equal(dv.gate(ctx, t[9], 0, ninl), want), (seed, case)
            G = PR.chain(t[9], F)
            G[1:, 4:] += rng.normal(0, 0.01, (F - 1, 3))       # (absolute poses that are not a chain of T_rel)
            got = dv.gate(ctx, G, 1, ninl)
            assert np.array_equal(got, [2] + [GR.gate(ninl[f - 1], G[f], G[f - 1]) for f in range(1, F)]), (seed, case)
            seen |= set(got.tolist())
        assert seen == {0, 1, 2}, seen
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(3))
def test_gated_map_builder_is_gated_builder(pkg, oracle, seed):
    """(b) vslam_build_windows_map_gated_dev(chain(T_rel), no index map, gate_states(T_rel, 0)) gives everything vslam_build_windows_gated_dev gives"""
    rng = np.random.default_rng(5200 + seed)
    ctx = pkg.VO(device=0, max_batch=1, pnp_reproj_thr=(4.0, 300.0, 1200.0)[seed])
    seen = set()
    try:
        for case in range(4):
            F = int(rng.integers(2, 40)); cap = int(rng.choice([64, 128])); n_kf = int(rng.integers(1, 11)); policy = case % 2
            t = list(dense_tracks(rng, F, cap) if case % 2 else _random_tracks(rng, F, cap, cap))
            t[9], ninl = _gate_inputs(rng, F, oracle)
            t = tuple(t)
            lm_cap, e_cap = F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1)
            if case == 3:
                lm_cap //= 8   # (the capacity cut: status bit 0, windows from the first that does not fit empty)
            want = _run_gated(pkg, ctx, t, ninl, n_kf, lm_cap, e_cap, policy)
            dv = _GDev(pkg, t)
            st = dv.gate(ctx, t[9], 0, ninl)
            got = dv.windows_gated(ctx, dv.chain(ctx), None, None, st, n_kf=n_kf, policy=policy, lm_cap=lm_cap, e_cap=e_cap)
            got["state"] = st
            _same(got, want, (seed, case))
            seen |= set(st.tolist())
        assert {1, 2} <= seen, seen
    finally:
        ctx.close()


@pytest.mark.parametrize("seed", range(2))
def test_every_state_2_is_ungated(pkg, seed):
    """(a) with every state 2 both gated builders give the ungated map entries' outputs, on pass-0 links and on a pass's index map"""
    rng = np.random.default_rng(5300 + seed)
    ctx = pkg.VO(device=0, max_batch=1, pnp_reproj_thr=(4.0, 300.0)[seed])
    try:
        for case in range(3):
            F = int(rng.integers(3, 20)); cap = int(rng.choice([64, 128])); n_kf = int(rng.integers(1, 11)); policy = case % 2
            t = dense_tracks(rng, F, cap)
            dv = _GDev(pkg, t)
            two = np.full(F, 2, np.int32)
            G = dv.chain(ctx)
            index, inl = None, None
            for k in range(2):
                a, b = dv.inputs_gated(ctx, G, index, inl, two), dv.inputs_gated(ctx, G, index, inl, two, gated=False)
                _same(a, b, (seed, case, k, "inputs"))
                wa = dv.windows_gated(ctx, G, index, inl, two, n_kf=n_kf, policy=policy)
                wb = dv.windows_gated(ctx, G, index, inl, two, n_kf=n_kf, policy=policy, gated=False)
                _same(wa, wb, (seed, case, k, "windows"))
                G, inl = _solve_host(a, G, GR.gate_solver)
                index = a["index"]
            assert a["n"].sum() > 0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. a host-driven pass loop
@pytest.mark.parametrize("seed", range(3))
def test_pass_loop_vs_restatement(pkg, seed):
    """passes 1 .. K on dense random tables with the gate stand-in solver run on the host between them: every pass's inputs and states against the
    restatement's, the final windows against its windows; K = F - 1 also against the sequential loop"""
    rng = np.random.default_rng(5400 + seed)
    ctx = pkg.VO(device=0, max_batch=1, pnp_reproj_thr=(4.0, 300.0, 4.0)[seed])
    flips, states = 0, set()
    try:
        for case in range(2):
            F = int(rng.integers(8, 13)); cap = int(rng.choice([128, 256])); n_kf = int(rng.integers(2, 11)); policy = case % 2
            t = dense_tracks(rng, F, cap)
            ninl0 = rng.integers(0, 200, F - 1)
            dv = _GDev(pkg, t)
            G0 = dv.chain(ctx)
            st0 = dv.gate(ctx, t[9], 0, ninl0)
            seq = GR.sequential(t, GR.gate_solver, n_kf=n_kf, policy=policy)
            for K in (1, 2, F - 1):
                tag = (seed, case, F, cap, K)
                ref = GR.passes(t, GR.gate_solver, K, ninl0, G0=G0, n_kf=n_kf, policy=policy, reproj_thr=ctx.params.pnp_reproj_thr)
                assert np.array_equal(st0, ref["state0"]), tag
                G, index, inl, st = G0, None, None, st0
                for k in range(K):
                    d_in = dv.inputs_gated(ctx, G, index, inl, st)
                    assert d_in["st"][0] == 0
                    _check_items(d_in, ref["per_pass"][k]["items"], tag + (k,))
                    G, inl = _solve_host(d_in, G, GR.gate_solver)
                    index = d_in["index"]
                    st_new = dv.gate(ctx, G, 1, inl.sum(1))
                    assert np.array_equal(st_new, ref["per_pass"][k]["state"]), (tag, k, st_new, ref["per_pass"][k]["state"])
                    flips += int((st_new != st).sum())
                    st = st_new
                assert np.array_equal(G, ref["G"]), tag
                w = dv.windows_gated(ctx, G, index, inl, st, n_kf=n_kf, policy=policy)
                assert w["st"][0] == ref["status"] and np.array_equal(w["kf_frame"], ref["kf_frame"]) and np.array_equal(w["evicted"], ref["evicted"]), tag
                assert np.array_equal(w["nkf"], ref["n_kf"]), tag
                assert KR.same_windows(_window_form(w, F), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
                states |= set(st.tolist())
                if K == F - 1:
                    assert np.array_equal(G, seq["G"]) and np.array_equal(st, seq["state"]), tag
                    for k_ in range(F - 1):
                        assert np.array_equal(index[k_], seq["items"][k_]["index"]) and np.array_equal(inl[k_, :seq["items"][k_]["n"]], seq["items"][k_]["mask"]), (tag, k_)
                    assert KR.same_windows(_window_form(w, F), seq["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
        assert {1, 2} <= states and flips > 0, (states, flips)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. the pipeline
def _replay(solved):
    """a solver that hands back the device's per-pass outputs: solved[k] = (G^k, inlier flags of pass k); the pass is counted from the item order"""
    calls = {"pass": 1, "i": -1}

    def solve(i, xyz, uv, guess):
        if i <= calls["i"]:
            calls["pass"] += 1
        calls["i"] = i
        T, inl = solved[calls["pass"]]
        return T[i + 1], inl[i, :len(uv)].astype(bool)
    return solve


def test_pipeline_per_pass_gate(pkg, oracle, synth):
    """16 rendered frames, RANSAC, K = 1, 2 and 15: the device's per-pass solver outputs replayed into the restatement reproduce its poses, masks, states
    and windows; K = 15 is the sequential loop; sampled items agree with oracle.pnp_ransac; the BA schedule runs on the windows; trajectory() gives the
    keyframes.  Pass k of a K-pass step is pass k of every longer one (the same stage A, a deterministic solver): one pipeline, stepped with K = 1 .. 15"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 16, 10
    seq = synth.stereo_sequence(B, seed=6)
    # (anms_num 1000: enough tracked features that some frames keep 80 inliers and are no keyframes; at 500 every frame has fewer)
    p = KeyframePipeline(B, anms_num=1000, n_kf=n_kf, unique_frames=B, seed=6, sequence=seq, ba_windows="tracks", pose="ransac", pose_inputs="map",
                         pose_passes=1, keyframe_gate="per_pass", window_policy="reference")
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
        for K in range(2, B):   # stage A is the same in every step
            for k in ("kps", "f2f", "inl", "Tpnp", "ninl"):
                assert np.array_equal(o1[k], outs[K][k]), (K, k)
        ninl0 = o1["ninl"][:B - 1]
        assert np.array_equal(o1["frame_state_prev"], GR.states0(t, ninl0))
        solved = {K: (outs[K]["T_c_w"], outs[K]["map_inl"]) for K in outs}
        G0 = _Dev(pkg, t).chain(p.vo)
        # RANSAC against the oracle on a sample of pass 1's items
        for i in (0, 5, B - 2):
            n = int(o1["map_n"][i])
            wT, winl, wn, _ = oracle.pnp_ransac(o1["map_xyz"][i, :n], o1["map_uv"][i, :n])
            assert np.array_equal(o1["map_inl"][i, :n], winl) and o1["map_ninl"][i] == wn, i
            if wn > 0:
                assert np.allclose(o1["T_c_w"][i + 1], wT, rtol=1e-4, atol=1e-6), i
        policy = 1
        for K in (1, 2, B - 1):
            o = outs[K]
            ref = GR.passes(t, _replay(solved), K, ninl0, G0=G0, n_kf=n_kf, policy=policy)
            assert np.array_equal(ref["G"], o["T_c_w"]), K
            for k in range(K):
                assert np.array_equal(ref["per_pass"][k]["state"], outs[k + 1]["frame_state"]), (K, k)
                assert np.array_equal(ref["per_pass"][k]["num_inliers"], outs[k + 1]["map_ninl"][:B - 1]), (K, k)
            assert np.array_equal(ref["state"], o["frame_state"]), K
            _check_items(dict(n=o["map_n"], index=o["map_index"], uv=o["map_uv"], xyz=o["map_xyz"]), ref["per_pass"][-1]["items"], K)
            g = dict(lm_off=o["ba_lm_off"], e_off=o["ba_e_off"], kf=o["ba_kf"], lm=o["ba_lm"], uv=o["ba_uv"], xyz=o["ba_xyz"], rel=o["ba_rel"])
            assert o["ba_build_status"][0] == ref["status"] and np.array_equal(o["ba_kf_frame"], ref["kf_frame"]), K
            assert np.array_equal(o["ba_evicted"], ref["evicted"]) and np.array_equal(o["ba_nkf"], ref["n_kf"]), K
            assert KR.same_windows(_window_form(g, B), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), K
        # K = F - 1: the sequential loop, whose solver outputs are the last pass's
        last = outs[B - 1]
        T15, inl15 = solved[B - 1]
        s = GR.sequential(t, lambda i, xyz, uv, guess: (T15[i + 1], inl15[i, :len(uv)].astype(bool)), n_kf=n_kf, policy=policy)
        assert np.array_equal(s["G"], last["T_c_w"]) and np.array_equal(s["state"], last["frame_state"])
        g = dict(lm_off=last["ba_lm_off"], e_off=last["ba_e_off"], kf=last["ba_kf"], lm=last["ba_lm"], uv=last["ba_uv"], xyz=last["ba_xyz"],
                 rel=last["ba_rel"])
        assert KR.same_windows(_window_form(g, B), s["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1])
        assert 2 <= (last["frame_state"] == 2).sum() < B, last["frame_state"]
        # the BA schedule on the last windows; the trajectory: the keyframes
        p.vo.ba_batch_dev(p.ba_batch, schedule=1)
        kf = np.flatnonzero(last["frame_state"] == 2)
        assert (p.vo.ba_status(B)[kf] == 0).all()
        ids, T = p.trajectory()
        assert sorted(ids.tolist()) == kf.tolist()
    finally:
        p.close()


def test_pipeline_per_pass_determinism_and_ring(synth):
    """two steps of one pipeline, and two pipelines of a PipelineRing, give bit-identical results"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline, PipelineRing
    B = 24
    kw = dict(anms_num=500, n_kf=10, unique_frames=8, seed=6, ba_windows="tracks", pose="ransac", pose_inputs="map", pose_passes=2,
              keyframe_gate="per_pass")
    ring = PipelineRing(2, B, **kw)
    solo = KeyframePipeline(B, sequence=ring.pipes[0].h_seq, **kw)
    try:
        ring.step(); ring.step()
        ring.sync()
        a, b = (p.download() for p in ring.pipes)
        solo.step()
        c = solo.download()
        solo.step()
        d = solo.download()
        keys = ("frame_state", "frame_state_prev", "map_n", "map_xyz", "map_uv", "map_index", "map_inl", "map_ninl", "T_c_w", "ba_lm_off", "ba_e_off",
                "ba_nkf", "ba_T", "ba_xyz", "ba_rel", "ba_inl", "ba_kf", "ba_lm", "ba_uv", "ba_kf_frame", "ba_evicted", "ba_build_status", "Tpnp", "inl")
        n_lm, n_e = a["ba_lm_off"][B], a["ba_e_off"][B]
        cut = dict(ba_xyz=n_lm, ba_rel=n_lm, ba_inl=n_lm, ba_kf=n_e, ba_lm=n_e, ba_uv=n_e)
        for k in keys:
            for other, tag in ((b, "ring"), (c, "solo"), (d, "rerun")):
                assert np.array_equal(a[k][:cut.get(k)], other[k][:cut.get(k)]), (tag, k)
        assert n_lm > 0 and (a["frame_state"] == 2).sum() >= 1
        ids, _ = ring.pipes[0].trajectory()
        assert sorted(ids.tolist()) == np.flatnonzero(a["frame_state"] == 2).tolist()
    finally:
        ring.close(); solo.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(pkg):
    import torch
    rng = np.random.default_rng(5500)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        F, cap = 5, 64
        t = _random_tracks(rng, F, cap, cap)
        dv = _GDev(pkg, t)
        G = torch.from_numpy(np.tile(KR.IDENT, (F, 1))).cuda()
        states = torch.full((F,), 2, dtype=torch.int32, device="cuda"); ninl = torch.full((F - 1,), 50, dtype=torch.int32, device="cuda")
        n_kf, lm_cap, e_cap = 4, F * cap * 5, F * cap * 10
        xyz = torch.zeros((F - 1, cap, 3), dtype=torch.float32, device="cuda"); uv = torch.zeros((F - 1, cap, 2), dtype=torch.float32, device="cuda")
        n = torch.zeros(F - 1, dtype=torch.int32, device="cuda"); index = torch.zeros((F - 1, cap), dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        o, bb = _outputs(pkg, F, n_kf, lm_cap, e_cap)
        torch.cuda.synchronize()

        def gate(F_=F, T_=G.data_ptr(), absolute=1, ninl_=ninl.data_ptr(), out=states.data_ptr()):
            ctx.gate_states_dev(F_, T_, absolute, ninl_, out)

        def inputs(out_cap=cap, G_=G.data_ptr(), state=states.data_ptr(), xyz_=xyz.data_ptr()):
            ctx.build_map_pnp_inputs_gated_dev(dv.tr, G_, None, state, xyz_, uv.data_ptr(), n.data_ptr(), index.data_ptr(), out_cap, st.data_ptr())

        def windows(G_=G.data_ptr(), state=states.data_ptr(), policy=0, n_kf_=n_kf, kf_frame=o["kf_frame"].data_ptr()):
            ctx.build_windows_map_gated_dev(dv.tr, G_, None, state, n_kf_, policy, 0.2, lm_cap, e_cap, bb, kf_frame, o["evicted"].data_ptr(),
                                            o["st"].data_ptr())
        gate(); gate(absolute=0); gate(F_=1, T_=None, ninl_=None); inputs(); windows(); windows(policy=1)   # (accepted; d_T_rel is NULL in dv.tr)
        ctx.sync()
        for call in (lambda: gate(absolute=2), lambda: gate(absolute=-1), lambda: gate(out=None), lambda: gate(T_=None), lambda: gate(ninl_=None),
                     lambda: gate(F_=0), lambda: inputs(state=None), lambda: inputs(out_cap=0), lambda: inputs(G_=None), lambda: inputs(xyz_=None),
                     lambda: windows(state=None), lambda: windows(G_=None), lambda: windows(policy=2), lambda: windows(n_kf_=0),
                     lambda: windows(kf_frame=None)):
            with pytest.raises(pkg.VslamError):
                call()
        chunk = torch.zeros((cap, 4), dtype=torch.float32, device="cuda")
        for member, val in (("d_T_abs", G.data_ptr()), ("d_carry_in", chunk.data_ptr()), ("d_carry_out", chunk.data_ptr())):
            setattr(dv.tr, member, val)
            if member == "d_carry_out":
                dv.tr.carry_out_frame = 1
            for call in (inputs, windows):
                with pytest.raises(pkg.VslamError):
                    call()
            setattr(dv.tr, member, None); dv.tr.carry_out_frame = 0
        inputs(); windows()
        ctx.sync()
    finally:
        ctx.close()
