"""The keyframe gate of insert_key_frame in throughput mode: vslam_build_windows_gated_dev (track_kernels.hip kf_gate_kernel, track_walk_kernel<true>,
kf_set_kernel<true> and the set-templated window kernels) against the CPU restatement of tests/kf_gate_ref.py, against vslam_build_windows_kf_dev
when every frame is a keyframe, and through KeyframePipeline(keyframe_gate=True).  Semantics: include/vslam_hip.h, vslam_build_windows_gated_dev."""
import math

import numpy as np
import pytest

import kf_gate_ref as R
from test_gpu_windows import _random_tracks
from test_gpu_windows_kf import _landmarks, _run
from test_kf_gate import HAND_STATE, hand_expected_sets, hand_table

pytestmark = pytest.mark.gpu


def _run_gated(pkg, ctx, tables, ninl, n_kf, lm_cap, e_cap, policy, near_dist=0.2, n_kf_arg=None, hook=None, null=()):
    """vslam_build_windows_gated_dev on host tables; every output array back on the host (unwritten entries keep their fill values)"""
    import torch
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = tables
    F, cap = kps.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [d(kps.view(np.uint8)), d(lr.view(np.uint8)), d(nlr), d(xyz), d(valid), d(rel), d(nk)]
    if F > 1:
        keep += [d(f2f.view(np.uint8)), d(nf2f), d(inl), d(T_rel), d(np.asarray(ninl, np.int32))]
    else:
        keep += [torch.zeros(16, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                 torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(7, dtype=torch.float64, device="cuda"),
                 torch.zeros(1, dtype=torch.int32, device="cuda")]
    t_kps, t_lr, t_nlr, t_xyz, t_valid, t_rel, t_nk, t_f2f, t_nf2f, t_inl, t_T, t_ninl = keep
    tr = pkg.TracksIn()
    tr.n_frames = F; tr.kp_capacity = cap; tr.lr_capacity = cap; tr.match_capacity = cap; tr.pnp_capacity = cap
    tr.d_kps = t_kps.data_ptr(); tr.d_lr = t_lr.data_ptr(); tr.d_nlr = t_nlr.data_ptr(); tr.d_xyz = t_xyz.data_ptr(); tr.d_valid = t_valid.data_ptr()
    tr.d_reliable = t_rel.data_ptr(); tr.d_f2f = t_f2f.data_ptr(); tr.d_nf2f = t_nf2f.data_ptr(); tr.d_pose_inlier = t_inl.data_ptr()
    tr.d_T_rel = t_T.data_ptr(); tr.d_nkps = t_nk.data_ptr()
    z = lambda n, dt, fill=0: torch.full(n if isinstance(n, tuple) else (n,), fill, dtype=dt, device="cuda")
    o = dict(lm_off=z(F + 1, torch.int32), e_off=z(F + 1, torch.int32), nkf=z(F, torch.int32, -5), T=z((F, n_kf, 7), torch.float64, -3.0),
             xyz=z((lm_cap, 3), torch.float32), rel=z(lm_cap, torch.uint8), inl=z(lm_cap, torch.uint8), kf=z(e_cap, torch.int32, -7),
             lm=z(e_cap, torch.int32), uv=z((e_cap, 2), torch.float32), st=z(1, torch.int32), kf_frame=z((F, n_kf), torch.int32, -9),
             evicted=z(F, torch.int32, -9), state=z(F, torch.int32, -9))
    bb = pkg.BaBatch()
    bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["e_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
    bb.d_reliable = o["rel"].data_ptr(); bb.d_lm_inlier = o["inl"].data_ptr(); bb.d_kf_idx = o["kf"].data_ptr(); bb.d_lm_idx = o["lm"].data_ptr()
    bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["nkf"].data_ptr()
    if hook is not None:
        hook(tr)
    ptr = lambda k, t: None if k in null else t.data_ptr()
    torch.cuda.synchronize()
    ctx.build_windows_gated_dev(tr, n_kf if n_kf_arg is None else n_kf_arg, policy, near_dist, ptr("ninl", t_ninl), lm_cap, e_cap, bb,
                                ptr("kf_frame", o["kf_frame"]), ptr("evicted", o["evicted"]), ptr("state", o["state"]), o["st"].data_ptr())
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _compare_gated(g, s, lm_cap, e_cap, n_kf, tag, xyz_tol=(3e-6, 2e-5)):
    """device output g against the restatement s: states, sets, status, offsets (capacity cut included), member counts, poses, windows"""
    wins, kf_frame, G = s["windows"], s["kf_frame"], s["G"]
    F = len(wins)
    assert np.array_equal(g["state"], s["state"]), (tag, g["state"], s["state"])
    assert np.array_equal(g["kf_frame"], kf_frame) and np.array_equal(g["evicted"], s["evicted"]), tag
    nl = np.array([len(w) for w in wins]); ne = np.array([sum(len(k) for k in w) for w in wins])
    il, ie = np.cumsum(nl), np.cumsum(ne)
    over = (il > lm_cap) | (ie > e_cap)
    fits = ~np.maximum.accumulate(over)
    lm_off = np.concatenate([[0], np.cumsum(np.where(fits, nl, 0))]); e_off = np.concatenate([[0], np.cumsum(np.where(fits, ne, 0))])
    assert g["st"][0] == int(over.any()) | s["status"], (tag, g["st"], s["status"])
    assert np.array_equal(g["lm_off"], lm_off) and np.array_equal(g["e_off"], e_off), tag
    assert np.array_equal(g["nkf"], s["n_kf"]), tag
    for b in range(F):
        if s["state"][b] != 2:
            assert np.allclose(g["T"][b][0], G[b], rtol=1e-9, atol=1e-11), (tag, b)   # slot 0: the frame's own pose
            assert (g["T"][b][1:] == -3.0).all(), (tag, b)                             # the other slots untouched
            continue
        S = kf_frame[b][kf_frame[b] >= 0]
        assert np.allclose(g["T"][b][:len(S)], G[S], rtol=1e-9, atol=1e-11), (tag, b)
        if not fits[b]:
            continue
        l0, l1, e0, e1 = lm_off[b], lm_off[b + 1], e_off[b], e_off[b + 1]
        kf, lm = g["kf"][e0:e1], g["lm"][e0:e1]
        cnt = np.bincount(lm, minlength=l1 - l0)
        assert (np.diff(cnt) >= 0).all() and (np.diff(lm) >= 0).all(), (tag, b)
        got = _landmarks(kf, lm, g["uv"][e0:e1], g["xyz"][l0:l1], g["rel"][l0:l1])
        assert got.keys() == wins[b].keys(), (tag, b, len(got), len(wins[b]))
        for k, (p, r) in wins[b].items():
            assert got[k][1] == r and np.allclose(got[k][0], p, rtol=xyz_tol[0], atol=xyz_tol[1]), (tag, b, k, got[k], p, r)
    assert (g["inl"][:lm_off[F]] == 1).all() and (g["kf"][e_off[F]:] == -7).all(), tag


def _roty(theta, t):
    return np.array([0.0, math.sin(theta / 2), 0.0, math.cos(theta / 2), t[0], t[1], t[2]])


def _gate_inputs(rng, F, O):
    """poses: short and long steps, yaw on both sides of +-0.03, a few motions with |log T| > 5; counts below 10, in 10..79 and >= 80"""
    T, n = [], []
    for _ in range(F - 1):
        u = rng.random()
        if u < 0.08:
            T.append(O.se3_exp(np.concatenate([rng.normal(0, 1, 3) / math.sqrt(3) * 6.5, rng.normal(0, 0.05, 3)])))   # too large a motion
        elif u < 0.5:
            T.append(_roty(rng.choice([-0.05, -0.01, 0.01, 0.05]) + rng.normal(0, 0.002), rng.normal(0, 0.05 if rng.random() < 0.5 else 0.5, 3)))
        else:
            s = 0.04 if rng.random() < 0.5 else 0.6
            T.append(O.se3_exp(np.concatenate([rng.normal(0, s, 3), rng.normal(0, s / 20, 3)])))
        n.append(int(rng.choice([rng.integers(0, 10), rng.integers(10, 80), rng.integers(80, 300), rng.integers(80, 300)])))
    return (np.stack(T) if T else np.zeros((0, 7))), np.array(n, np.int32)


@pytest.mark.parametrize("seed", range(3))
def test_random_tables_vs_restatement(pkg, oracle, seed):
    """random tables and gate inputs, both policies, both track rules, n_kf 1..12, capacity overflow: every output against the restatement"""
    rng = np.random.default_rng(8100 + seed)
    rule = 1 if seed < 2 else 0
    ctxs = {thr: pkg.VO(device=0, max_batch=1, pnp_reproj_thr=thr) for thr in (4.0, 300.0)}
    for c_ in ctxs.values():
        c_.set_tuning(track_rule=rule)
    seen = np.zeros(3, int); n_rej_runs = 0
    try:
        for case in range(8):
            thr = (4.0, 300.0)[case % 2]; ctx = ctxs[thr]; policy = case % 2 if seed != 1 else 1 - case % 2
            F = int(rng.integers(1, 40)); cap = int(rng.choice([64, 100, 256])); n_kf = int(rng.integers(1, 13))
            tables = list(_random_tracks(rng, F, cap, int(rng.integers(1, cap + 1))))
            tables[9], ninl = _gate_inputs(rng, F, oracle)
            s = R.simulate(tables, ninl, n_kf, policy, reproj_thr=thr, track_rule=rule)
            assert s["margin"] > 1e-9, (seed, case, s["margin"])
            for f in range(1, F):   # the restated rule is the oracle's
                want = 0 if not oracle.check_motion(int(ninl[f - 1]), tables[9][f - 1], 1.0) else \
                    (1 if ninl[f - 1] >= 80 and oracle.se3_angle_y(tables[9][f - 1]) < 0.03 else 2)
                assert s["state"][f] == want
            seen += np.bincount(s["state"], minlength=3)
            n_rej_runs += int(s["status"] & 4 != 0)
            nl_tot = sum(len(w) for w in s["windows"]); ne_tot = sum(sum(len(k) for k in w) for w in s["windows"])
            shrink = rng.random() < 0.3 and nl_tot > 4
            lm_cap = max(int(nl_tot * rng.uniform(0.3, 0.9)), 1) if shrink else nl_tot + 7
            e_cap = ne_tot + 5
            g = _run_gated(pkg, ctx, tables, ninl, n_kf, lm_cap, e_cap, policy)
            _compare_gated(g, s, lm_cap, e_cap, n_kf, (seed, case, F, cap, n_kf, policy, shrink))
        assert (seen > 0).all() and n_rej_runs > 0, (seen, n_rej_runs)
    finally:
        for c_ in ctxs.values():
            c_.close()


@pytest.mark.parametrize("policy", (0, 1))
def test_hand_worked_table_on_device(pkg, policy):
    tables, ninl = hand_table()
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        g = _run_gated(pkg, ctx, tables, ninl, 3, 64, 128, policy)
        s = R.simulate(tables, ninl, 3, policy)
        kf, ev = hand_expected_sets(policy)
        assert g["state"].tolist() == HAND_STATE and np.array_equal(g["kf_frame"], kf) and np.array_equal(g["evicted"], ev) and g["st"][0] == 4
        _compare_gated(g, s, 64, 128, 3, ("hand", policy))
    finally:
        ctx.close()


def test_all_keyframes_bit_identical_to_kf_dev(pkg, oracle):
    """every frame a keyframe (10..79 inliers, motions inside the check): every output of the gated call is vslam_build_windows_kf_dev's with the
    same policy, bit for bit"""
    rng = np.random.default_rng(91)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        for case in range(6):
            F = int(rng.integers(1, 40)); cap = int(rng.choice([64, 256])); n_kf = int(rng.integers(1, 13))
            tables = list(_random_tracks(rng, F, cap, int(rng.integers(1, cap + 1))))
            if case % 2:
                tables[9] = np.stack([oracle.se3_exp(np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.003, 3)])) for _ in range(F - 1)]) \
                    if F > 1 else np.zeros((0, 7))
            ninl = rng.integers(10, 80, max(F - 1, 0))
            lm_cap, e_cap = F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1)
            if case == 4:
                lm_cap //= 3 * n_kf   # (the capacity cut as well)
            for policy in (0, 1):
                ref = _run(pkg, ctx, tables, n_kf, lm_cap, e_cap, policy=policy)
                g = _run_gated(pkg, ctx, tables, ninl, n_kf, lm_cap, e_cap, policy)
                assert (g["state"] == 2).all(), (case, policy)
                for k in ref:
                    assert np.array_equal(g[k], ref[k]), (case, policy, k)
    finally:
        ctx.close()


def test_refusals(pkg):
    """a chunk, a NULL d_num_inliers (n_frames > 1), NULL d_kf_frame / d_evicted / d_frame_state, a policy other than 0 / 1, a NaN or negative
    near_dist, n_kf outside 1..VSLAM_MAX_KF: VSLAM_ERR_ARG"""
    import torch
    rng = np.random.default_rng(4)
    tables = _random_tracks(rng, 6, 64, 40)
    ninl = np.full(5, 50, np.int32)
    ctx = pkg.VO(device=0, max_batch=1)
    T_abs = torch.zeros((6, 7), dtype=torch.float64, device="cuda"); T_abs[:, 3] = 1
    carry = torch.zeros((64, 4), dtype=torch.float32, device="cuda")

    def chunk(member):
        def hook(tr):
            if member == "d_T_abs":
                tr.d_T_abs = T_abs.data_ptr()
            elif member == "d_carry_in":
                tr.d_carry_in = carry.data_ptr()
            else:
                tr.d_carry_out = carry.data_ptr(); tr.carry_out_frame = 3
        return hook
    try:
        for policy in (0, 1):
            g = _run_gated(pkg, ctx, tables, ninl, 4, 4096, 8192, policy)   # (valid: each case below differs in one argument)
            assert g["st"][0] == 0 and (g["state"] == 2).all()
        cases = [dict(near_dist=float("nan")), dict(near_dist=-0.1), dict(policy=2), dict(policy=-1), dict(n_kf_arg=0), dict(n_kf_arg=13)]
        cases += [dict(hook=chunk(m)) for m in ("d_T_abs", "d_carry_in", "d_carry_out")]
        cases += [dict(null=(k,)) for k in ("ninl", "kf_frame", "evicted", "state")]
        for kw in cases:
            kw.setdefault("policy", 1)
            with pytest.raises(pkg.VslamError):
                _run_gated(pkg, ctx, tables, ninl, 4, 4096, 8192, **kw)
        one = [t[:1] for t in tables[:6]] + [t[:0] for t in tables[6:10]] + [tables[10][:1]]
        g = _run_gated(pkg, ctx, one, np.zeros(0, np.int32), 4, 4096, 8192, 1, null=("ninl",))   # (one frame: no count to read)
        assert g["state"].tolist() == [2] and g["st"][0] == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------ rendered frames through KeyframePipeline
def _built_tables(built, B):
    return (built["kps"][:B], built["lr"], built["nlr"], built["xyz"], built["valid"], built["rel"], built["f2f"][:B - 1], built["nf2f"][:B - 1],
            built["inl"][:B - 1], built["Tpnp"][:B - 1], built["cnt"][:B])


def _ba_compacted(pkg, pipe, built, K):
    """one BA call over only the windows K (keyframe steps), built on the host from the downloaded window arrays"""
    import torch
    B = pipe.B
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(pipe.dev)
    lm_off = np.concatenate([built["ba_lm_off"][K], built["ba_lm_off"][B:]]).astype(np.int32)
    e_off = np.concatenate([built["ba_e_off"][K], built["ba_e_off"][B:]]).astype(np.int32)
    t = dict(lm_off=d(lm_off), e_off=d(e_off), T=d(built["ba_T"][K]), nkf=d(built["ba_nkf"][K]), xyz=d(built["ba_xyz"]), rel=d(built["ba_rel"]),
             inl=d(built["ba_inl"]), kf=d(built["ba_kf"]), lm=d(built["ba_lm"]), uv=d(built["ba_uv"]))
    bb = pkg.BaBatch()
    bb.n_windows = len(K); bb.n_kf = pipe.n_kf
    bb.d_lm_off = t["lm_off"].data_ptr(); bb.d_edge_off = t["e_off"].data_ptr(); bb.d_T_c_w = t["T"].data_ptr(); bb.d_xyz = t["xyz"].data_ptr()
    bb.d_reliable = t["rel"].data_ptr(); bb.d_lm_inlier = t["inl"].data_ptr(); bb.d_kf_idx = t["kf"].data_ptr(); bb.d_lm_idx = t["lm"].data_ptr()
    bb.d_uv = t["uv"].data_ptr(); bb.d_n_kf = t["nkf"].data_ptr(); bb.d_chi2 = None; bb.d_stats = None; bb.K4 = None
    bb.total_lm = pipe.lm_capacity; bb.total_edge = pipe.edge_capacity
    torch.cuda.synchronize(pipe.dev)
    pipe.vo.ba_batch_dev(bb, schedule=1)
    pipe.vo.sync()
    torch.cuda.synchronize(pipe.dev)
    return t["T"].cpu().numpy(), t["inl"].cpu().numpy()


@pytest.mark.parametrize("window_policy", ("sliding", "reference"))
def test_pipeline_keyframe_gate(pkg, oracle, window_policy):
    """rendered frames (ping-pong over 8; the sequence yaws by less than 0.03 per frame): the pose stage's counts are set to at most 60 on every third
    frame and at least 100 on the others, so that keyframes and tracked frames alternate.  States against the rule on the downloaded counts and poses, windows against the restatement on the downloaded tables, the BA of
    the keyframe windows against one BA call over only them, the trajectory (keyframes only, in write order)"""
    import torch
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 24, 4
    policy = 1 if window_policy == "reference" else 0
    pipe = KeyframePipeline(B, anms_num=500, n_kf=n_kf, unique_frames=8, seed=6, ba_windows="tracks", window_policy=window_policy,
                            keyframe_gate=True)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track()
        with torch.cuda.stream(pipe.stream):
            pipe.d_ninl[0::3].clamp_(min=100); pipe.d_ninl[1::3].clamp_(min=100); pipe.d_ninl[2::3].clamp_(max=60)
        pipe.stage_build_windows()
        built = pipe.download()
        st = built["frame_state"]
        ninl, Tp = built["ninl"][:B - 1], built["Tpnp"][:B - 1]
        want = [2] + [0 if not oracle.check_motion(int(ninl[i]), Tp[i], 1.0) else (1 if ninl[i] >= 80 and oracle.se3_angle_y(Tp[i]) < 0.03 else 2)
                      for i in range(B - 1)]
        assert st.tolist() == want
        K = np.flatnonzero(st == 2)
        assert 3 <= len(K) < B, st
        s = R.simulate(_built_tables(built, B), ninl, n_kf, policy)
        assert s["margin"] > 1e-9
        g = dict(lm_off=built["ba_lm_off"], e_off=built["ba_e_off"], nkf=built["ba_nkf"], T=built["ba_T"], xyz=built["ba_xyz"], rel=built["ba_rel"],
                 inl=built["ba_inl"], kf=built["ba_kf"].copy(), lm=built["ba_lm"], uv=built["ba_uv"], st=built["ba_build_status"],
                 kf_frame=built["ba_kf_frame"], evicted=built["ba_evicted"], state=st)
        g["kf"][g["e_off"][B]:] = -7
        g["T"] = g["T"].copy(); g["T"][st != 2, 1:] = -3.0   # (the pipeline's pose slots are not pre-filled)
        _compare_gated(g, s, pipe.lm_capacity, pipe.edge_capacity, n_kf, ("pipe", window_policy), xyz_tol=(3e-6, 2e-5))
        # the BA schedule over all B windows; the keyframe windows' results against one call over only them
        pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        done = pipe.download()
        T_c, inl_c = _ba_compacted(pkg, pipe, built, K)
        assert np.array_equal(done["ba_T"][K], T_c)
        assert np.array_equal(done["ba_inl"][:built["ba_lm_off"][B]], inl_c[:built["ba_lm_off"][B]])
        # the trajectory: every keyframe once, evicted ones at their eviction, each from the last keyframe window that held it
        ids, T = pipe.trajectory()
        kf, ev = built["ba_kf_frame"], built["ba_evicted"]
        last = K[-1]
        order = [int(e) for e in ev if e >= 0] + [int(f) for f in kf[last] if f >= 0]
        assert ids.tolist() == order and sorted(order) == K.tolist()
        for f, t in zip(ids, T):
            w = max(x for x in K if f in kf[x])
            assert np.array_equal(t, done["ba_T"][w][int(np.flatnonzero(kf[w] == f)[0])]), f
    finally:
        pipe.close()


def test_pipeline_gate_ring_and_rerun(synth):
    """two gated pipelines in a PipelineRing over the same frames, and a second step of one: bit-identical results"""
    from stereo_visual_slam_amd.pipeline import PipelineRing
    B = 24
    ring = PipelineRing(2, B, anms_num=500, n_kf=10, unique_frames=8, seed=6, ba_windows="tracks", window_policy="reference", keyframe_gate=True)
    try:
        ring.step(); ring.step()
        ring.sync()
        a, b = (p.download() for p in ring.pipes)
        keys = ("frame_state", "ba_kf_frame", "ba_evicted", "ba_lm_off", "ba_e_off", "ba_nkf", "ba_T", "ba_xyz", "ba_rel", "ba_inl", "ba_kf", "ba_lm",
                "ba_uv", "ba_build_status", "ninl", "Tpnp")
        n_lm, n_e = a["ba_lm_off"][B], a["ba_e_off"][B]
        cut = dict(ba_xyz=n_lm, ba_rel=n_lm, ba_inl=n_lm, ba_kf=n_e, ba_lm=n_e, ba_uv=n_e)
        for k in keys:
            assert np.array_equal(a[k][:cut.get(k)], b[k][:cut.get(k)]), k
        assert (a["frame_state"] == 2).sum() >= 1
        ring.pipes[0].step()
        c = ring.pipes[0].download()
        for k in keys:
            assert np.array_equal(a[k][:cut.get(k)], c[k][:cut.get(k)]), ("rerun", k)
        ids, _ = ring.pipes[0].trajectory()
        assert sorted(ids.tolist()) == np.flatnonzero(a["frame_state"] == 2).tolist()
    finally:
        ring.close()
