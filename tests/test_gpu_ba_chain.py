"""The chained BA of throughput mode on rendered inputs: the landmark ids the window builders write (vslam_set_window_ids), vslam_ba_chain_dev against
the numpy step composer of tests/ba_chain_ref.py -- bit for bit with vslam_ba_batch_dev(schedule = 1) as the composer's optimiser, within the schedule
tests' tolerance with the oracle's --, the trajectory it leaves, and what it refuses.  Contract: include/vslam_hip.h, vslam_ba_chain_dev."""
import numpy as np
import pytest

import ba_chain_ref as CR

pytestmark = pytest.mark.gpu

B, N_KF, ANMS = 24, 10, 500
SEGMENTS = (13, 1, 12)
BATCH_KEYS = ("ba_lm_off", "ba_e_off", "ba_nkf", "ba_T", "ba_xyz", "ba_rel", "ba_inl", "ba_kf", "ba_lm", "ba_uv", "ba_build_status", "ba_kf_frame", "ba_evicted")

CONFIGS = {
    "sliding": dict(kw=dict(), min_kf=10),
    "reference": dict(kw=dict(window_policy="reference"), min_kf=10),
    # (anms_num 1000 / RANSAC as in tests/test_gpu_gated_map.py: at 500 no frame keeps the 80 inliers that make a non-keyframe; min_kf 3 so that the few
    # keyframes of a gated run give pass-through windows AND active ones)
    "gate": dict(kw=dict(keyframe_gate="per_pass", pose_inputs="map", pose_passes=2, pose="ransac", anms_num=1000), min_kf=3),
    "segments1": dict(kw=dict(segments=SEGMENTS), min_kf=1),
    "segments10": dict(kw=dict(segments=SEGMENTS), min_kf=10),
}


@pytest.fixture(scope="module")
def seq8(synth):
    return synth.stereo_sequence(8, seed=6)


def _batch_of(out):
    return dict(n_kf=N_KF, lm_off=out["ba_lm_off"], e_off=out["ba_e_off"], nkf=out["ba_nkf"], T=out["ba_T"], xyz=out["ba_xyz"], rel=out["ba_rel"],
                inl=out["ba_inl"], kf=out["ba_kf"], lm=out["ba_lm"], uv=out["ba_uv"])


class _BatchRunner:
    """compose() callback: upload the staging batch into buffers of the pipeline's capacities, vslam_ba_batch_dev(schedule = 1), download"""

    def __init__(self, pkg, pipe, n_slots):
        import torch
        self.torch, self.pipe = torch, pipe
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=pipe.dev)
        L, E = pipe.lm_capacity, pipe.edge_capacity
        self.t = dict(lm_off=z(n_slots + 1, torch.int32), e_off=z(n_slots + 1, torch.int32), nkf=z(n_slots, torch.int32), T=z((n_slots, N_KF, 7), torch.float64),
                      xyz=z((L, 3), torch.float32), rel=z(L, torch.uint8), inl=z(L, torch.uint8), kf=z(E, torch.int32), lm=z(E, torch.int32), uv=z((E, 2), torch.float32))
        bb = pkg.BaBatch()
        t = self.t
        bb.n_kf = N_KF; bb.d_lm_off = t["lm_off"].data_ptr(); bb.d_edge_off = t["e_off"].data_ptr(); bb.d_T_c_w = t["T"].data_ptr(); bb.d_xyz = t["xyz"].data_ptr()
        bb.d_reliable = t["rel"].data_ptr(); bb.d_lm_inlier = t["inl"].data_ptr(); bb.d_kf_idx = t["kf"].data_ptr(); bb.d_lm_idx = t["lm"].data_ptr()
        bb.d_uv = t["uv"].data_ptr(); bb.d_chi2 = None; bb.d_stats = None; bb.K4 = None; bb.d_n_kf = t["nkf"].data_ptr()
        bb.total_lm = L; bb.total_edge = E
        self.bb = bb

    def __call__(self, st):
        torch, t, n = self.torch, self.t, st["n_windows"]
        with torch.cuda.stream(self.pipe.stream):
            for k in ("lm_off", "e_off", "nkf", "T", "xyz", "rel", "inl", "kf", "lm", "uv"):
                a = torch.from_numpy(np.ascontiguousarray(st[k]))
                t[k][:len(a)].copy_(a.to(self.pipe.dev))
        self.pipe.stream.synchronize()
        self.bb.n_windows = n
        self.pipe.vo.ba_batch_dev(self.bb, schedule=1)
        status = self.pipe.vo.ba_status(n)
        return dict(T=t["T"][:n].cpu().numpy(), inl=t["inl"].cpu().numpy(), status=status)


_CASES = {}


def _case(pkg, seq8, name):
    """one pipeline per configuration: the built windows with their ids, the independent BA on them, the chained BA on them (with status, ran and the
    trajectory it leaves).  Computed once and shared by the tests; nothing in it is modified afterwards."""
    if name in _CASES:
        return _CASES[name]
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    cfg = CONFIGS[name]
    kw = dict(anms_num=ANMS, n_kf=N_KF, unique_frames=8, seed=6, ba_windows="tracks", ba_chain=True, ba_chain_min_kf=cfg["min_kf"])
    kw.update(cfg["kw"])
    if "segments" in kw:
        kw["segment_sequences"] = [seq8 if n > 1 else seq8[:1] for n in SEGMENTS]
    else:
        kw["sequence"] = seq8
    nb = sum(SEGMENTS) if "segments" in kw else B   # (the segmented batch: 26 frames)
    pipe = KeyframePipeline(nb, **kw)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        built = pipe.download()
        pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        indep = pipe.download()
        indep_status = pipe.vo.ba_status(nb)
        pipe.stage_ba()   # (builds again -- the same windows -- and chains)
        chained = pipe.download()
        status = pipe.vo.ba_status(nb)
        traj = pipe.trajectory() if pipe.seg_first is None else pipe.trajectories()
        first = np.array([0, nb]) if pipe.seg_first is None else pipe.seg_first
        kf_frame = None if pipe._chain_kf_frame() is None else built["ba_kf_frame"]
        n_slots = len(first) - 1
        ref = CR.compose(_batch_of(built), built["ba_lm_id"], kf_frame, first, cfg["min_kf"], _BatchRunner(pkg, pipe, n_slots))
    finally:
        pipe.close()
    _CASES[name] = dict(built=built, indep=indep, indep_status=indep_status, chained=chained, status=status, traj=traj, first=first, ref=ref,
                        min_kf=cfg["min_kf"], cap=pipe.cap, B=nb)
    return _CASES[name]


# ------------------------------------------------------------------ 1. ids
def test_ids(pkg, oracle, seq8):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    pipe = KeyframePipeline(B, anms_num=ANMS, n_kf=N_KF, unique_frames=8, seed=6, sequence=seq8, ba_windows="tracks", window_policy="reference", ba_chain=True)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        o = pipe.download()
        pipe.vo.set_window_ids(None)   # the same call without an id buffer
        pipe.stage_build_windows()
        plain = pipe.download()
        pipe.vo.set_window_ids(pipe.ba_lm_id.data_ptr(), pipe.lm_capacity)
    finally:
        pipe.close()
    for k in BATCH_KEYS:
        assert np.array_equal(o[k], plain[k]), k
    cap = pipe.cap
    lm_off, e_off, kf_frame, ids, kps = o["ba_lm_off"], o["ba_e_off"], o["ba_kf_frame"], o["ba_lm_id"], o["kps"]
    assert o["ba_build_status"][0] == 0 and lm_off[B] > 0
    full = oracle.build_windows(o["kps"][:B], o["lr"], o["nlr"], o["xyz"], o["valid"], o["rel"], o["f2f"][:B - 1], o["nf2f"][:B - 1], o["inl"][:B - 1],
                                o["Tpnp"][:B - 1], n_kf=B)
    l0, e0, e1 = full["lm_off"][B - 1], full["edge_off"][B - 1], full["edge_off"][B]
    lm_of_obs = {}   # (two keypoints of a frame -- other octaves -- can share a pixel: an observation then names more than one candidate)
    for f, l, (u, v) in zip(full["kf_idx"][e0:e1], full["lm_idx"][e0:e1], full["uv"][e0:e1]):
        lm_of_obs.setdefault((int(f), float(u), float(v)), set()).add(int(l))
    oracle_of_id, id_of_oracle = {}, {}
    n_ambiguous = 0
    for w in range(B):
        S = kf_frame[w][kf_frame[w] >= 0]
        wid = ids[lm_off[w]:lm_off[w + 1]]
        assert len(np.unique(wid)) == len(wid), w   # distinct inside a window
        assert (wid >= 0).all() and (wid < B * cap).all(), w
        kf, lm, uv = o["ba_kf"][e_off[w]:e_off[w + 1]], o["ba_lm"][e_off[w]:e_off[w + 1]], o["ba_uv"][e_off[w]:e_off[w + 1]]
        by_lm = {}
        for k_, l_, (u, v) in zip(kf, lm, uv):
            by_lm.setdefault(int(l_), []).append((int(S[k_]), float(u), float(v)))
        for l, i in enumerate(wid):
            f, kp = divmod(int(i), cap)
            if f in S:   # the creating keypoint is one of the window's observations of the landmark
                assert (f, float(kps[f][kp]["x"]), float(kps[f][kp]["y"])) in by_lm[l], (w, l, f, kp)
            ol = set.intersection(*[lm_of_obs[obs] for obs in by_lm[l]])
            assert len(ol) >= 1, (w, l)
            if len(ol) > 1:
                n_ambiguous += 1
                continue
            ol = ol.pop()
            assert oracle_of_id.setdefault(int(i), ol) == ol and id_of_oracle.setdefault(ol, int(i)) == int(i), (w, l, i, ol)
    assert n_ambiguous * 50 < lm_off[B], n_ambiguous
    assert len(oracle_of_id) < lm_off[B]   # (landmarks do recur across windows: the identity is worth something)


# ------------------------------------------------------------------ 2. the chain contract, bit for bit
@pytest.mark.parametrize("name", list(CONFIGS))
def test_chain_equals_composer(pkg, seq8, name):
    c = _case(pkg, seq8, name)
    built, chained, ref, nb = c["built"], c["chained"], c["ref"], c["B"]
    for k in BATCH_KEYS:   # the chain run rebuilt the same windows
        if k not in ("ba_T", "ba_inl"):
            assert np.array_equal(built[k], chained[k]), (name, k)
    n_lm = built["ba_lm_off"][nb]
    assert np.array_equal(chained["ba_ran"], ref["ran"]), (name, chained["ba_ran"], ref["ran"])
    assert np.array_equal(c["status"], ref["status"]), name
    nkf = built["ba_nkf"]
    for w in range(nb):   # (slots beyond a window's keyframes are nobody's)
        assert np.array_equal(chained["ba_T"][w][:max(nkf[w], 1)].view(np.uint64), ref["T"][w][:max(nkf[w], 1)].view(np.uint64)), (name, w)
    assert np.array_equal(chained["ba_inl"][:n_lm], ref["inl"][:n_lm]), name
    active = np.flatnonzero(ref["ran"])
    assert len(active) >= 2 and (c["status"][active] == 0).all(), (name, active)
    assert (ref["ran"] == ((nkf >= c["min_kf"]) & (nkf >= 1))).all()
    # guard: the chain is not the independent launch
    ind = c["indep"]
    assert any(not np.array_equal(chained["ba_T"][w][:nkf[w]], ind["ba_T"][w][:nkf[w]]) for w in active), name
    assert not np.array_equal(chained["ba_inl"][:n_lm], ind["ba_inl"][:n_lm]), name
    if name == "gate":
        st = built["frame_state"]
        lo, hi = active.min(), active.max()
        assert (st[lo:hi + 1] != 2).any(), st   # a non-keyframe step inside the chained range
        assert (nkf[st != 2] == 0).all() and (chained["ba_ran"][st != 2] == 0).all()
        assert ((nkf > 0) & (nkf < c["min_kf"])).any()   # and pass-through windows
    if name.startswith("segments"):
        assert [s["n_windows"] for s in ref["steps"]] == [3] + [2] * 11 + [1]


# ------------------------------------------------------------------ 3. against the oracle
def test_chain_vs_oracle(pkg, oracle, seq8):
    """B = 14, min_kf = 10, one sequence: windows 9..13 run chained.  Flags compound over the steps, so the oracle run must not classify any edge
    within 1e-6 (relative) of its threshold.  Smallest margin seen with seed 6 over the 20 classifications of the five steps: 2.838e-03."""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    n = 14
    pipe = KeyframePipeline(n, anms_num=ANMS, n_kf=N_KF, unique_frames=8, seed=6, sequence=seq8, ba_windows="tracks", ba_chain=True)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        built = pipe.download()
        pipe.stage_ba()
        got = pipe.download()
        assert (pipe.vo.ba_status(n) == 0).all()
    finally:
        pipe.close()
    margins = []
    ref = CR.compose(_batch_of(built), built["ba_lm_id"], None, [0, n], N_KF, CR.oracle_run(oracle, margins))
    print("smallest |chi2 - threshold| / threshold over %d classifications: %.3e" % (len(margins), min(margins)))
    assert min(margins) >= 1e-6, min(margins)
    assert ref["ran"].tolist() == [0] * 9 + [1] * 5 and np.array_equal(got["ba_ran"], ref["ran"])
    n_lm = built["ba_lm_off"][n]
    for w in range(n):
        nk = int(built["ba_nkf"][w])
        assert np.allclose(got["ba_T"][w][:nk], ref["T"][w][:nk], rtol=1e-4, atol=1e-6), (w, np.abs(got["ba_T"][w][:nk] - ref["T"][w][:nk]).max())
    assert np.array_equal(got["ba_inl"][:n_lm], ref["inl"][:n_lm]), int((got["ba_inl"][:n_lm] != ref["inl"][:n_lm]).sum())
    assert (ref["inl"][:n_lm] == 0).any()


# ------------------------------------------------------------------ 4. trajectory
def test_trajectory(pkg, seq8):
    c = _case(pkg, seq8, "sliding")
    ids, T = c["traj"]
    from stereo_visual_slam_amd.trajectory import sliding_keyframes
    kf, _ = sliding_keyframes(B, N_KF)
    assert sorted(ids.tolist()) == list(range(B))
    ran = c["chained"]["ba_ran"]
    differs = 0
    for f, t in zip(ids, T):
        holders = [w for w in range(B) if f in kf[w]]
        w = max(holders); k = int(np.flatnonzero(kf[w] == f)[0])
        assert np.array_equal(t, c["chained"]["ba_T"][w][k]), f
        if sum(int(ran[x]) for x in holders) >= 2:
            assert not np.array_equal(t, c["indep"]["ba_T"][w][k]), f
            differs += 1
    assert differs >= 10
    s = _case(pkg, seq8, "segments10")   # per segment: the same rule with the segment's own frame ids
    assert [len(i) for i, _ in s["traj"]] == list(SEGMENTS)


# ------------------------------------------------------------------ 5. refusals
def test_refusals(pkg, seq8):
    import torch
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    n = 12
    pipe = KeyframePipeline(n, anms_num=ANMS, n_kf=N_KF, unique_frames=8, seed=6, sequence=seq8, ba_windows="tracks", ba_chain=True, ba_chain_min_kf=1)
    vo, tr = pipe.vo, pipe.tracks
    ids = pipe.ba_lm_id.data_ptr()
    T_abs = torch.zeros((n, 7), dtype=torch.float64, device=pipe.dev); T_abs[:, 3] = 1

    def chunk():
        tr.d_T_abs = T_abs.data_ptr()
        try:
            pipe.stage_build_windows()
        finally:
            tr.d_T_abs = None

    def small_ids():
        vo.set_window_ids(ids, pipe.lm_capacity - 1)
        try:
            pipe.stage_build_windows()
        finally:
            vo.set_window_ids(ids, pipe.lm_capacity)

    def wrong_table():
        vo.set_segments([0, 5, n - 1])
        try:
            vo.ba_chain_dev(pipe.ba_batch, ids, None, 1, None)
        finally:
            vo.set_segments(None)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track()
        pipe.stage_ba(); vo.sync()   # (valid)
        cases = [lambda: vo.ba_chain_dev(pipe.ba_batch, None, None, 1, None), lambda: vo.ba_chain_dev(pipe.ba_batch, ids, None, 0, None),
                 lambda: vo.ba_chain_dev(pipe.ba_batch, ids, None, N_KF + 1, None), wrong_table, small_ids, chunk]
        for i, call in enumerate(cases):
            with pytest.raises(pkg.VslamError) as e:
                call()
            msg = str(e.value)
            assert "(%d)" % pkg.VSLAM_ERR_ARG in msg and len(msg.split("): ", 1)[1]) > 8, (i, msg)
            pipe.stage_ba(); vo.sync()   # a following valid call succeeds
            assert (vo.ba_status(n) == 0).all() and pipe.ba_ran.cpu().numpy().all(), i
    finally:
        pipe.close()
