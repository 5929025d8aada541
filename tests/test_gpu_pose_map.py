"""Pose inputs against the map (pose_inputs="map"): vslam_chain_poses_dev, vslam_build_map_pnp_inputs_dev (track_link_kernel<true>,
track_map_inputs_kernel) and vslam_build_windows_map_dev against vslam_build_windows_kf_dev, against the CPU restatement of tests/pose_map_ref.py
(the pass semantics and the sequential loop), and through KeyframePipeline(pose_inputs="map").  Semantics: include/vslam_hip.h."""
import numpy as np
import pytest

import kf_gate_ref as KR
import pose_map_ref as R
from test_gpu_windows import _random_tracks
from test_gpu_windows_kf import _landmarks, _run

pytestmark = pytest.mark.gpu
XYZ_TOL = (3e-6, 2e-5)   # (test_gpu_kf_gate.py's position tolerance: device double arithmetic vs numpy)


class _Dev:
    """host tables on the device, and the three entries on them"""

    def __init__(self, pkg, tables):
        import torch
        self.torch, self.pkg, self.t = torch, pkg, tables
        kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = tables
        self.F, self.cap = kps.shape
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.keep = dict(kps=d(kps.view(np.uint8)), lr=d(lr.view(np.uint8)), nlr=d(nlr), xyz=d(xyz), valid=d(valid), rel=d(rel), nk=d(nk),
                         f2f=d(f2f.view(np.uint8)), nf2f=d(nf2f), inl=d(inl), T=d(T_rel))
        k = self.keep
        tr = pkg.TracksIn()
        tr.n_frames = self.F; tr.kp_capacity = self.cap; tr.lr_capacity = self.cap; tr.match_capacity = self.cap; tr.pnp_capacity = self.cap
        tr.d_kps = k["kps"].data_ptr(); tr.d_lr = k["lr"].data_ptr(); tr.d_nlr = k["nlr"].data_ptr(); tr.d_xyz = k["xyz"].data_ptr()
        tr.d_valid = k["valid"].data_ptr(); tr.d_reliable = k["rel"].data_ptr(); tr.d_f2f = k["f2f"].data_ptr(); tr.d_nf2f = k["nf2f"].data_ptr()
        tr.d_pose_inlier = k["inl"].data_ptr(); tr.d_T_rel = None; tr.d_nkps = k["nk"].data_ptr()
        self.tr = tr

    def chain(self, ctx):
        G = self.torch.zeros((self.F, 7), dtype=self.torch.float64, device="cuda")
        self.torch.cuda.synchronize()
        ctx.chain_poses_dev(self.F, self.keep["T"].data_ptr(), G.data_ptr())
        ctx.sync()
        return G.cpu().numpy()

    def inputs(self, ctx, G, index_prev=None, inl_prev=None, out_cap=None):
        """one pass: G (F x 7) host, index_prev / inl_prev host arrays of the previous pass (None: pass 0, the tables' own-depth flags)"""
        torch, F, cap = self.torch, self.F, self.cap
        out_cap = cap if out_cap is None else out_cap
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        tG = d(G)
        t_idx = None if index_prev is None else d(index_prev.astype(np.int32))
        t_inl = self.keep["inl"] if inl_prev is None else d(inl_prev.astype(np.uint8))
        self.tr.d_pose_inlier = t_inl.data_ptr(); self.tr.pnp_capacity = cap if inl_prev is None else inl_prev.shape[1]
        o = dict(xyz=torch.full((F - 1, out_cap, 3), -5.0, dtype=torch.float32, device="cuda"), uv=torch.full((F - 1, out_cap, 2), -5.0, device="cuda"),
                 n=torch.full((F - 1,), -5, dtype=torch.int32, device="cuda"), index=torch.full((F - 1, cap), -5, dtype=torch.int32, device="cuda"),
                 st=torch.full((1,), -5, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        ctx.build_map_pnp_inputs_dev(self.tr, tG.data_ptr(), None if t_idx is None else t_idx.data_ptr(), o["xyz"].data_ptr(), o["uv"].data_ptr(),
                                     o["n"].data_ptr(), o["index"].data_ptr(), out_cap, o["st"].data_ptr())
        ctx.sync()
        self.tr.d_pose_inlier = self.keep["inl"].data_ptr(); self.tr.pnp_capacity = cap
        return {k: v.cpu().numpy() for k, v in o.items()}

    def windows(self, ctx, G, index=None, inl=None, n_kf=10, policy=0, lm_cap=None, e_cap=None):
        """vslam_build_windows_map_dev; every output back on the host (the layout of test_gpu_windows_kf._run)"""
        torch, F, cap = self.torch, self.F, self.cap
        lm_cap = F * cap * (n_kf + 1) if lm_cap is None else lm_cap
        e_cap = 2 * F * cap * (n_kf + 1) if e_cap is None else e_cap
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        tG = d(G)
        t_idx = None if index is None else d(index.astype(np.int32))
        t_inl = self.keep["inl"] if inl is None else d(inl.astype(np.uint8))
        self.tr.d_pose_inlier = t_inl.data_ptr(); self.tr.pnp_capacity = cap if inl is None else inl.shape[1]
        o, bb = _window_outputs(self.pkg, F, n_kf, lm_cap, e_cap)
        torch.cuda.synchronize()
        ctx.build_windows_map_dev(self.tr, tG.data_ptr(), None if t_idx is None else t_idx.data_ptr(), n_kf, policy, 0.2, lm_cap, e_cap, bb,
                                  o["kf_frame"].data_ptr(), o["evicted"].data_ptr(), o["st"].data_ptr())
        ctx.sync()
        self.tr.d_pose_inlier = self.keep["inl"].data_ptr(); self.tr.pnp_capacity = cap
        return {k: v.cpu().numpy() for k, v in o.items()}


def _window_outputs(pkg, F, n_kf, lm_cap, e_cap):
    """the output arrays of one window build (the layout of test_gpu_windows_kf._run) and the BaBatch that points at them"""
    import torch
    z = lambda n, dt, fill=0: torch.full(n if isinstance(n, tuple) else (n,), fill, dtype=dt, device="cuda")
    o = dict(lm_off=z(F + 1, torch.int32), e_off=z(F + 1, torch.int32), nkf=z(F, torch.int32), T=z((F, n_kf, 7), torch.float64),
             xyz=z((lm_cap, 3), torch.float32), rel=z(lm_cap, torch.uint8), inl=z(lm_cap, torch.uint8), kf=z(e_cap, torch.int32, -7),
             lm=z(e_cap, torch.int32), uv=z((e_cap, 2), torch.float32), st=z(1, torch.int32), kf_frame=z((F, n_kf), torch.int32, -9),
             evicted=z(F, torch.int32, -9))
    bb = pkg.BaBatch()
    bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["e_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
    bb.d_reliable = o["rel"].data_ptr(); bb.d_lm_inlier = o["inl"].data_ptr(); bb.d_kf_idx = o["kf"].data_ptr(); bb.d_lm_idx = o["lm"].data_ptr()
    bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["nkf"].data_ptr()
    return o, bb


def _window_form(g, F):
    """device windows in the comparison form of kf_gate_ref"""
    out = []
    for b in range(F):
        l0, l1, e0, e1 = g["lm_off"][b], g["lm_off"][b + 1], g["e_off"][b], g["e_off"][b + 1]
        out.append(_landmarks(g["kf"][e0:e1], g["lm"][e0:e1], g["uv"][e0:e1], g["xyz"][l0:l1], g["rel"][l0:l1]))
    return out


def _check_items(dev, items, tag):
    """device inputs of one pass against the restatement's: counts, index maps and uv exact, positions within the tolerance"""
    for i, it in enumerate(items):
        n = it["n"]
        assert dev["n"][i] == n, (tag, i, dev["n"][i], n)
        assert np.array_equal(dev["index"][i], it["index"]), (tag, i)
        assert np.array_equal(dev["uv"][i, :n], it["uv"]), (tag, i)
        assert np.allclose(dev["xyz"][i, :n], it["xyz"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), (tag, i)


def _solve_host(dev_in, G_prev, solver):
    """the stand-in solver on the device's inputs, with the failure rule: G^k and the inlier flags of every item"""
    F = len(G_prev)
    G = G_prev.copy(); G[0] = KR.IDENT
    inl = np.zeros((F - 1, dev_in["xyz"].shape[1]), np.uint8)
    for i in range(F - 1):
        n = int(dev_in["n"][i])
        T, m = solver(i, dev_in["xyz"][i, :n], dev_in["uv"][i, :n], G_prev[i + 1])
        m = np.asarray(m, bool)
        if m.any():
            G[i + 1] = T; inl[i, :n] = m
        else:
            G[i + 1] = G_prev[i]
    return G, inl


# ------------------------------------------------------------------ 1. the builder contract
@pytest.mark.parametrize("seed", range(3))
def test_map_builder_pass0_is_kf_dev_bit_for_bit(pkg, seed):
    rng = np.random.default_rng(4100 + seed)
    ctx = pkg.VO(device=0, max_batch=1, pnp_reproj_thr=(4.0, 300.0, 1200.0)[seed])
    try:
        for case in range(4):
            F = int(rng.integers(2, 30)); cap = int(rng.choice([64, 100, 256])); n_kf = int(rng.integers(1, 11)); policy = case % 2
            t = _random_tracks(rng, F, cap, int(rng.integers(1, cap + 1)))
            lm_cap, e_cap = F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1)
            want = _run(pkg, ctx, t, n_kf, lm_cap, e_cap, policy=policy)
            dv = _Dev(pkg, t)
            got = dv.windows(ctx, dv.chain(ctx), None, None, n_kf=n_kf, policy=policy, lm_cap=lm_cap, e_cap=e_cap)
            for k in want:
                assert np.array_equal(got[k], want[k]), (seed, case, k)
    finally:
        ctx.close()


def test_chain_is_the_builders(pkg):
    """vslam_chain_poses_dev: the builders' poses (window slot k of the sliding window = G[s + k]), bit for bit; G_0 = identity"""
    rng = np.random.default_rng(4200)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        F, cap, n_kf = 300, 64, 10   # (more than one 256-frame scan chunk)
        t = _random_tracks(rng, F, cap, 8)
        want = _run(pkg, ctx, t, n_kf, F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1), policy=0)
        G = _Dev(pkg, t).chain(ctx)
        assert np.array_equal(G[0], KR.IDENT)
        for b in range(F):
            s = max(0, b - n_kf + 1)
            assert np.array_equal(want["T"][b][:b - s + 1], G[s:b + 1]), b
        assert np.allclose(G, R.chain(t[9], F), rtol=1e-9, atol=1e-9)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2-4. the inputs entry and a device-driven pass loop
@pytest.mark.parametrize("seed", range(3))
def test_pass_loop_vs_restatement(pkg, seed):
    """passes 1 .. K on random tables with the stand-in solver run on the host between them: every pass's inputs against the restatement's, the
    final windows against its windows; K = F - 1 also against the sequential loop; every input's position is its landmark's in window i, bit for bit"""
    _pass_loop_vs_restatement(pkg, seed, (4.0, 300.0, 4.0)[seed])


def _pass_loop_vs_restatement(pkg, seed, thr, cam=None):
    """cam (fx, fy, cx, cy, b): the context's camera, its K handed to the restatement (None: the KITTI camera of both).  Returns the number of
    entries of the first two passes' input lists (counts and index maps) in which the restatement under that camera differs from the restatement
    under the KITTI camera."""
    rng = np.random.default_rng(4300 + seed)
    ctx = pkg.VO(device=0, max_batch=1, pnp_reproj_thr=thr, **({} if cam is None else dict(cam=cam)))
    kw = {} if cam is None else dict(K=np.asarray(cam, np.float64)[:4])
    n_inputs = n_camera_inputs = 0
    try:
        for case in range(2):
            F = int(rng.integers(10, 14)); cap = int(rng.choice([64, 128])); n_kf = int(rng.integers(2, 11)); policy = case % 2
            t = _random_tracks(rng, F, cap, cap)
            dv = _Dev(pkg, t)
            G0 = dv.chain(ctx)
            seq = R.sequential(t, R.standin_solver, n_kf=n_kf, policy=policy)
            for K in (1, 2, F - 1):
                tag = (seed, case, F, cap, K)
                ref = R.passes(t, R.standin_solver, K, G0=G0, n_kf=n_kf, policy=policy, reproj_thr=ctx.params.pnp_reproj_thr, **kw)
                if cam is not None and K == 2:
                    kitti = R.passes(t, R.standin_solver, K, G0=G0, n_kf=n_kf, policy=policy, reproj_thr=ctx.params.pnp_reproj_thr)
                    n_camera_inputs += sum(abs(a["n"] - b["n"]) + int((a["index"] != b["index"]).sum())
                                           for k in range(K) for a, b in zip(ref["per_pass"][k]["items"], kitti["per_pass"][k]["items"]))
                G, index, inl = G0, None, None
                for k in range(K):
                    d_in = dv.inputs(ctx, G, index, inl)
                    assert d_in["st"][0] == 0
                    _check_items(d_in, ref["per_pass"][k]["items"], tag + (k,))
                    n_inputs += int(d_in["n"].sum())
                    if k == 0:   # (4) positions: bit for bit those of window i on the same poses and links (sliding, every frame's landmarks)
                        w = dv.windows(ctx, G, index, inl, n_kf=n_kf, policy=0)
                        f2f = t[6]
                        for i in range(F - 1):
                            s = max(0, i - n_kf + 1); l0, e0, e1 = w["lm_off"][i], w["e_off"][i], w["e_off"][i + 1]
                            kf, lm, uv = w["kf"][e0:e1], w["lm"][e0:e1], w["uv"][e0:e1]
                            for kk in np.flatnonzero(d_in["index"][i] >= 0):
                                j, q = d_in["index"][i][kk], f2f["queryIdx"][i, kk]
                                x, y = t[0]["x"][i, q], t[0]["y"][i, q]
                                e = np.flatnonzero((kf == i - s) & (uv[:, 0] == x) & (uv[:, 1] == y))
                                assert len(e) == 1, (tag, i, kk)
                                assert np.array_equal(w["xyz"][l0 + lm[e[0]]], d_in["xyz"][i, j]), (tag, i, kk)
                    G, inl = _solve_host(d_in, G, R.standin_solver)
                    index = d_in["index"]
                assert np.array_equal(G, ref["G"]), tag
                w = dv.windows(ctx, G, index, inl, n_kf=n_kf, policy=policy)
                assert w["st"][0] == ref["status"] and np.array_equal(w["kf_frame"], ref["kf_frame"]) and np.array_equal(w["evicted"], ref["evicted"]), tag
                assert KR.same_windows(_window_form(w, F), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
                if K == F - 1:   # the sequential loop (its poses do not depend on the chain of T_rel)
                    assert np.array_equal(G, seq["G"]), tag
                    for k_ in range(F - 1):
                        assert np.array_equal(d_in["index"][k_], seq["items"][k_]["index"]) and np.array_equal(inl[k_, :seq["items"][k_]["n"]], seq["items"][k_]["mask"]), (tag, k_)
                    assert KR.same_windows(_window_form(w, F), seq["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), tag
        assert n_inputs > 200, n_inputs
    finally:
        ctx.close()
    return n_camera_inputs


def test_inputs_capacity_cut(pkg):
    """out_capacity smaller than an item's list: the first out_capacity inputs are kept, the rest map to -1, status bit 0"""
    rng = np.random.default_rng(4400)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        F, cap = 6, 64
        t = _random_tracks(rng, F, cap, cap)
        dv = _Dev(pkg, t)
        G0 = dv.chain(ctx)
        full = dv.inputs(ctx, G0)
        oc = max(1, int(full["n"].max()) // 2)
        cut = dv.inputs(ctx, G0, out_cap=oc)
        assert full["st"][0] == 0 and cut["st"][0] == 1
        assert np.array_equal(cut["n"], np.minimum(full["n"], oc))
        assert np.array_equal(cut["index"], np.where(full["index"] < oc, full["index"], -1))
        for i in range(F - 1):
            n = int(cut["n"][i])
            assert np.array_equal(cut["uv"][i, :n], full["uv"][i, :n]) and np.array_equal(cut["xyz"][i, :n], full["xyz"][i, :n])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 5-6. the pipeline
def _tables(out, B):
    return (out["kps"][:B], out["lr"], out["nlr"], out["xyz"], out["valid"], out["rel"], out["f2f"][:B - 1], out["nf2f"][:B - 1], out["inl"][:B - 1],
            out["Tpnp"][:B - 1], out["cnt"][:B])


@pytest.mark.parametrize("pose", ("ransac", "lm"))
def test_pipeline_map_passes(pkg, oracle, synth, pose):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 16, 10
    seq = synth.stereo_sequence(B, seed=6)
    outs, pipes = {}, {}
    try:
        for K in (1, 2):
            pipes[K] = p = KeyframePipeline(B, anms_num=500, n_kf=n_kf, unique_frames=B, seed=6, sequence=seq, ba_windows="tracks", pose=pose,
                                            pose_inputs="map", pose_passes=K, window_policy="reference" if K == 2 else "sliding")
            p.stage_orb(); p.stage_stereo_match(); p.stage_track(); p.stage_build_windows()
            outs[K] = p.download()
        o1, o2 = outs[1], outs[2]
        t = _tables(o1, B)
        for k in ("kps", "f2f", "inl", "Tpnp", "ninl"):   # stage A is the same in both pipelines, and keeps its meaning
            assert np.array_equal(o1[k], o2[k]), k
        G0 = _Dev(pkg, t).chain(pipes[1].vo)
        # pass 1 contains every stage-A input match, and its count is the matches out of a feature of the own-depth walk
        ref0 = R._walk(t, G0, decide=R.pass0_links(t), n_kf=1)["items"]
        k2lr = np.full((B, pipes[1].cap), -1)
        for f in range(B):
            n = int(o1["nlr"][f]); k2lr[f, o1["lr"]["queryIdx"][f, :n]] = np.arange(n)
        for i in range(B - 1):
            n = int(o1["nf2f"][i]); q = o1["f2f"]["queryIdx"][i, :n]
            own = (k2lr[i, q] >= 0) & (o1["valid"][i, np.maximum(k2lr[i, q], 0)] != 0)
            assert own.sum() == o1["pn"][i] and (o1["map_index"][i, :n][own] >= 0).all(), i
            assert o1["map_n"][i] == ref0[i]["n"] and np.array_equal(o1["map_index"][i], ref0[i]["index"]), i
        assert (o1["map_n"][:B - 1] > o1["pn"][:B - 1]).mean() > 0.5, (o1["map_n"], o1["pn"])
        # the device solver on the emitted inputs: RANSAC against the oracle on a sample of items
        if pose == "ransac":
            for i in (0, 5, B - 2):
                n = int(o1["map_n"][i])
                wT, winl, wn, _ = oracle.pnp_ransac(o1["map_xyz"][i, :n], o1["map_uv"][i, :n])
                assert np.array_equal(o1["map_inl"][i, :n], winl) and o1["map_ninl"][i] == wn, i
                if wn > 0:
                    assert np.allclose(o1["T_c_w"][i + 1], wT, rtol=1e-4, atol=1e-6), i
        # the final windows: the restatement fed with the device's per-pass solver outputs
        solved = {1: (o1["T_c_w"], o1["map_inl"]), 2: (o2["T_c_w"], o2["map_inl"])}
        for K, o in ((1, o1), (2, o2)):
            calls = {"pass": 1, "i": -1}

            def replay(i, xyz, uv, guess):   # (pass k of the K = 2 pipeline is the K = 1 pipeline's for k = 1: the same stage A, the same solver)
                if i <= calls["i"]:
                    calls["pass"] += 1
                calls["i"] = i
                T, inl = solved[calls["pass"]]
                return T[i + 1], inl[i, :len(uv)].astype(bool)
            ref = R.passes(t, replay, K, G0=G0, n_kf=n_kf, policy=1 if K == 2 else 0)
            assert np.array_equal(ref["G"], o["T_c_w"]), K
            _check_items(dict(n=o["map_n"], index=o["map_index"], uv=o["map_uv"], xyz=o["map_xyz"]), ref["per_pass"][-1]["items"], K)
            g = dict(lm_off=o["ba_lm_off"], e_off=o["ba_e_off"], kf=o["ba_kf"], lm=o["ba_lm"], uv=o["ba_uv"], xyz=o["ba_xyz"], rel=o["ba_rel"])
            assert o["ba_build_status"][0] == 0 and np.array_equal(o["ba_kf_frame"], ref["kf_frame"])
            assert KR.same_windows(_window_form(g, B), ref["windows"], rtol=XYZ_TOL[0], atol=XYZ_TOL[1]), K
        # the BA schedule on the windows
        for K in (1, 2):
            pipes[K].vo.ba_batch_dev(pipes[K].ba_batch, schedule=1)
            assert (pipes[K].vo.ba_status(B) == 0).all(), K
            ids, T = pipes[K].trajectory()
            assert sorted(ids.tolist()) == list(range(B))
    finally:
        for p in pipes.values():
            p.close()


def test_pipeline_map_determinism_and_ring(synth):
    """two steps of one pipeline, and two pipelines of a PipelineRing, give bit-identical results"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline, PipelineRing
    B = 24
    kw = dict(anms_num=500, n_kf=10, unique_frames=8, seed=6, ba_windows="tracks", pose="ransac", pose_inputs="map", pose_passes=2)
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
        keys = ("map_n", "map_xyz", "map_uv", "map_index", "map_inl", "map_ninl", "T_c_w", "ba_lm_off", "ba_e_off", "ba_T", "ba_xyz", "ba_rel", "ba_inl",
                "ba_kf", "ba_lm", "ba_uv", "ba_kf_frame", "Tpnp", "inl")
        n_lm, n_e = a["ba_lm_off"][B], a["ba_e_off"][B]
        cut = dict(ba_xyz=n_lm, ba_rel=n_lm, ba_inl=n_lm, ba_kf=n_e, ba_lm=n_e, ba_uv=n_e)
        for k in keys:
            for other, tag in ((b, "ring"), (c, "solo"), (d, "rerun")):
                assert np.array_equal(a[k][:cut.get(k)], other[k][:cut.get(k)]), (tag, k)
        assert n_lm > 0 and a["map_n"][:B - 1].sum() > 0
    finally:
        ring.close(); solo.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals(pkg):
    import torch
    rng = np.random.default_rng(4500)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        F, cap = 5, 64
        t = _random_tracks(rng, F, cap, cap)
        dv = _Dev(pkg, t)
        G = torch.from_numpy(np.tile(KR.IDENT, (F, 1))).cuda()
        n_kf, lm_cap, e_cap = 4, F * cap * 5, F * cap * 10
        xyz = torch.zeros((F - 1, cap, 3), dtype=torch.float32, device="cuda"); uv = torch.zeros((F - 1, cap, 2), dtype=torch.float32, device="cuda")
        n = torch.zeros(F - 1, dtype=torch.int32, device="cuda"); index = torch.zeros((F - 1, cap), dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        o, bb = _window_outputs(pkg, F, n_kf, lm_cap, e_cap)
        torch.cuda.synchronize()

        def inputs(out_cap=cap, G_=G.data_ptr(), xyz_=xyz.data_ptr()):
            ctx.build_map_pnp_inputs_dev(dv.tr, G_, None, xyz_, uv.data_ptr(), n.data_ptr(), index.data_ptr(), out_cap, st.data_ptr())

        def windows(G_=G.data_ptr(), policy=0):
            ctx.build_windows_map_dev(dv.tr, G_, None, n_kf, policy, 0.2, lm_cap, e_cap, bb, o["kf_frame"].data_ptr(), o["evicted"].data_ptr(),
                                      o["st"].data_ptr())
        inputs(); windows(); windows(policy=1)   # (accepted: d_T_rel is NULL in dv.tr, the map entries do not need it)
        ctx.sync()
        for call in (lambda: inputs(out_cap=0), lambda: inputs(G_=None), lambda: inputs(xyz_=None), lambda: windows(G_=None), lambda: windows(policy=2)):
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
        with pytest.raises(pkg.VslamError):
            ctx.chain_poses_dev(F, dv.keep["T"].data_ptr(), None)
        inputs()
        ctx.sync()
    finally:
        ctx.close()
