"""Keyframe culling in throughput mode: vslam_build_windows_kf_dev (track_kernels.hip kf_band_kernel / kf_set_kernel and the set-templated window
kernels) against a numpy restatement of Map::remove_keyframe (map.cpp:48-130) on the chained poses, and the windows against oracle/windows.c's
full-history windows restricted to the surviving keyframes.  Semantics: include/vslam_hip.h, vslam_build_windows_kf_dev."""
import numpy as np
import pytest

from test_gpu_windows import _random_tracks

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ expected keyframe sets
def _chain(O, T_rel):
    G = [np.array([0, 0, 0, 1, 0, 0, 0], np.float64)]
    for T in T_rel:
        G.append(O.se3_mul(T, G[-1]))
    return np.stack(G)


def _ref_keyframes(O, T_rel, n_kf, near_dist=0.2):
    """kf_frame (B, n_kf), evicted (B,), and the smallest margin of any decision (how far a distance was from flipping it)"""
    G = _chain(O, T_rel)
    B = len(G)
    kf = np.full((B, n_kf), -1, np.int32); ev = np.full(B, -1, np.int32)
    S = [0]; kf[0, 0] = 0; margin = np.inf
    for b in range(1, B):
        S = S + [b]
        if len(S) > n_kf:
            Gi = O.se3_inv(G[b])
            d = np.array([np.linalg.norm(O.se3_log(O.se3_mul(G[k], Gi))) for k in S[:-1]])
            far, far_d, near, near_d = None, 0.0, None, 1e6
            for k, dk in zip(S[:-1], d):
                if dk > far_d:
                    far, far_d = k, dk
                if dk < near_d:
                    near, near_d = k, dk
            e = near if near is not None and near_d < near_dist else far
            if len(d) > 1:
                srt = np.sort(d)
                margin = min(margin, srt[1] - srt[0], srt[-1] - srt[-2])
            margin = min(margin, abs(near_d - near_dist))
            S.remove(e); ev[b] = e
        kf[b, :len(S)] = S
    return kf, ev, margin


# ------------------------------------------------------------------ device runs
def _run(pkg, ctx, tables, n_kf, lm_cap, e_cap, policy=1, near_dist=0.2, use_nkps=True, legacy=False, n_kf_arg=None, hook=None):
    import torch
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = tables
    F, cap = kps.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [d(kps.view(np.uint8)), d(lr.view(np.uint8)), d(nlr), d(xyz), d(valid), d(rel), d(nk)]
    keep += [d(f2f.view(np.uint8)), d(nf2f), d(inl), d(T_rel)] if F > 1 else [torch.zeros(16, dtype=torch.uint8, device="cuda"),
                                                                             torch.zeros(1, dtype=torch.int32, device="cuda"),
                                                                             torch.zeros(1, dtype=torch.uint8, device="cuda"),
                                                                             torch.zeros(7, dtype=torch.float64, device="cuda")]
    t_kps, t_lr, t_nlr, t_xyz, t_valid, t_rel, t_nk, t_f2f, t_nf2f, t_inl, t_T = keep
    tr = pkg.TracksIn()
    tr.n_frames = F; tr.kp_capacity = cap; tr.lr_capacity = cap; tr.match_capacity = cap; tr.pnp_capacity = cap
    tr.d_kps = t_kps.data_ptr(); tr.d_lr = t_lr.data_ptr(); tr.d_nlr = t_nlr.data_ptr(); tr.d_xyz = t_xyz.data_ptr(); tr.d_valid = t_valid.data_ptr()
    tr.d_reliable = t_rel.data_ptr(); tr.d_f2f = t_f2f.data_ptr(); tr.d_nf2f = t_nf2f.data_ptr(); tr.d_pose_inlier = t_inl.data_ptr()
    tr.d_T_rel = t_T.data_ptr(); tr.d_nkps = t_nk.data_ptr() if use_nkps else None
    z = lambda n, dt, fill=0: torch.full(n if isinstance(n, tuple) else (n,), fill, dtype=dt, device="cuda")
    o = dict(lm_off=z(F + 1, torch.int32), e_off=z(F + 1, torch.int32), nkf=z(F, torch.int32), T=z((F, n_kf, 7), torch.float64),
             xyz=z((lm_cap, 3), torch.float32), rel=z(lm_cap, torch.uint8), inl=z(lm_cap, torch.uint8), kf=z(e_cap, torch.int32, -7),
             lm=z(e_cap, torch.int32), uv=z((e_cap, 2), torch.float32), st=z(1, torch.int32), kf_frame=z((F, n_kf), torch.int32, -9),
             evicted=z(F, torch.int32, -9))
    bb = pkg.BaBatch()
    bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["e_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
    bb.d_reliable = o["rel"].data_ptr(); bb.d_lm_inlier = o["inl"].data_ptr(); bb.d_kf_idx = o["kf"].data_ptr(); bb.d_lm_idx = o["lm"].data_ptr()
    bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["nkf"].data_ptr()
    if hook is not None:
        hook(tr)
    torch.cuda.synchronize()
    if legacy:
        ctx.build_windows_dev(tr, n_kf, lm_cap, e_cap, bb, o["st"].data_ptr())
    else:
        ctx.build_windows_kf_dev(tr, n_kf if n_kf_arg is None else n_kf_arg, policy, near_dist, lm_cap, e_cap, bb, o["kf_frame"].data_ptr(), o["evicted"].data_ptr(), o["st"].data_ptr())
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in o.items()}


# ------------------------------------------------------------------ window comparison
def _landmarks(kf_idx, lm_idx, uv, xyz, rel):
    """one window's landmarks, order-free: {sorted observations (slot, u, v): (position, reliable)}"""
    out = {}
    for l in range(len(xyz)):
        sel = lm_idx == l
        key = tuple(sorted(zip(kf_idx[sel].tolist(), uv[sel, 0].tolist(), uv[sel, 1].tolist())))
        assert key and key not in out
        out[key] = (xyz[l], int(rel[l]))
    return out


def _expected_windows(full, kf_frame):
    """oracle windows with n_kf = F (window b = frames [0, b] as of time b, kf_idx = frame) restricted to S_b: observations in culled frames
    dropped, landmarks left without one dropped, kf_idx remapped to the slot"""
    F = len(kf_frame)
    wins = []
    for b in range(F):
        S = [int(f) for f in kf_frame[b] if f >= 0]
        slot = {f: k for k, f in enumerate(S)}
        l0, l1, e0, e1 = full["lm_off"][b], full["lm_off"][b + 1], full["edge_off"][b], full["edge_off"][b + 1]
        kf, lm, uv = full["kf_idx"][e0:e1], full["lm_idx"][e0:e1], full["uv"][e0:e1]
        keep = np.isin(kf, S)
        lms = {}
        for l in np.unique(lm[keep]):
            sel = keep & (lm == l)
            key = tuple(sorted(zip([slot[int(f)] for f in kf[sel]], uv[sel, 0].tolist(), uv[sel, 1].tolist())))
            lms[key] = (full["xyz"][l0 + l], int(full["reliable"][l0 + l]))
        wins.append(lms)
    return wins


def _compare(g, wins, kf_frame, lm_cap, e_cap, G, tag, xyz_tol=(3e-6, 2e-5)):
    F = len(wins)
    nl = np.array([len(w) for w in wins]); ne = np.array([sum(len(k) for k in w) for w in wins])
    il, ie = np.cumsum(nl), np.cumsum(ne)
    over = (il > lm_cap) | (ie > e_cap)
    fits = ~np.maximum.accumulate(over)
    lm_off = np.concatenate([[0], np.cumsum(np.where(fits, nl, 0))]); e_off = np.concatenate([[0], np.cumsum(np.where(fits, ne, 0))])
    assert (g["st"][0] & 1) == int(over.any()), tag
    assert np.array_equal(g["lm_off"], lm_off) and np.array_equal(g["e_off"], e_off), tag
    assert np.array_equal(g["nkf"], (kf_frame >= 0).sum(1)), tag
    for b in range(F):
        S = kf_frame[b][kf_frame[b] >= 0]
        assert np.allclose(g["T"][b][:len(S)], G[S], rtol=1e-9, atol=1e-11), (tag, b)
        if not fits[b]:
            continue
        l0, l1, e0, e1 = lm_off[b], lm_off[b + 1], e_off[b], e_off[b + 1]
        kf, lm = g["kf"][e0:e1], g["lm"][e0:e1]
        cnt = np.bincount(lm, minlength=l1 - l0)
        assert (np.diff(cnt) >= 0).all() and (np.diff(lm) >= 0).all(), (tag, b)   # landmark-major, by observation count
        got = _landmarks(kf, lm, g["uv"][e0:e1], g["xyz"][l0:l1], g["rel"][l0:l1])
        assert got.keys() == wins[b].keys(), (tag, b, len(got), len(wins[b]))
        for k, (p, r) in wins[b].items():
            assert got[k][1] == r and np.allclose(got[k][0], p, rtol=xyz_tol[0], atol=xyz_tol[1]), (tag, b, k, got[k], p, r)
    assert (g["inl"][:lm_off[F]] == 1).all() and (g["kf"][e_off[F]:] == -7).all(), tag


def _z_steps(z):
    """T_rel of pure z translations: the chained pose of frame f translates by z[f]"""
    T = np.zeros((len(z) - 1, 7)); T[:, 3] = 1; T[:, 6] = np.diff(z)
    return T


# ------------------------------------------------------------------ tests
def test_hand_worked_eviction(pkg, oracle):
    """pure z translations, n_kf = 3: d = |z_b - z_k|.  Near-evictions at steps 4, 5, 7; the oldest frame is the farthest at 3 and 6; at 8 the
    farthest is frame 6, not the oldest (sliding would evict 5)"""
    z = [0, 1, 2, 3, 3.1, 3.15, 4.15, 3.05, 0.5]
    rng = np.random.default_rng(11)
    tables = list(_random_tracks(rng, len(z), 64, 48))
    tables[9] = _z_steps(np.array(z, np.float64))
    want_ev = [-1, -1, -1, 0, 3, 4, 1, 5, 6]
    want_kf = [[0, -1, -1], [0, 1, -1], [0, 1, 2], [1, 2, 3], [1, 2, 4], [1, 2, 5], [2, 5, 6], [2, 6, 7], [2, 7, 8]]
    kf, ev, margin = _ref_keyframes(oracle, tables[9], 3)
    assert ev.tolist() == want_ev and kf.tolist() == want_kf and margin > 1e-9
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        g = _run(pkg, ctx, tables, 3, 64 * 9 * 4, 64 * 9 * 8)
        assert g["evicted"].tolist() == want_ev and g["kf_frame"].tolist() == want_kf and g["st"][0] == 0
        full = oracle.build_windows(*tables[:10], n_kf=len(z), lm_capacity=64 * 9 * 10, edge_capacity=64 * 9 * 20)
        _compare(g, _expected_windows(full, kf), kf, 64 * 9 * 4, 64 * 9 * 8, _chain(oracle, tables[9]), "hand")
    finally:
        ctx.close()


def _random_T_rel(rng, F, O):
    """steps of both kinds: short ones (the nearest frame closer than 0.2: near-evictions) and long ones, in random directions (reversals: the
    farthest frame need not be the oldest)"""
    out = []
    for _ in range(F - 1):
        s = 0.04 if rng.random() < 0.5 else 0.6
        out.append(O.se3_exp(np.concatenate([rng.normal(0, s, 3), rng.normal(0, s / 20, 3)])))
    return np.stack(out) if out else np.zeros((0, 7))


@pytest.mark.parametrize("seed", range(4))
def test_random_tracks_vs_oracle(pkg, oracle, seed):
    """random association / match / flag tables and random poses with both eviction branches, both track rules, thresholds 4 / 300 / 1200 px,
    n_kf 1..12, capacity overflow: the sets against the numpy rule, the windows against the oracle's full-history windows restricted to them"""
    _random_tracks_kf_vs_oracle(pkg, oracle, seed)


def _random_tracks_kf_vs_oracle(pkg, oracle, seed, thrs=(4.0, 300.0, 1200.0), cam=None):
    """cam (fx, fy, cx, cy, b): the contexts' camera, its K handed to the oracle (None: the KITTI camera of both).  Returns the number of edges by
    which the oracle's full-history windows under that camera differ from those under the KITTI camera, summed over the cases."""
    rng = np.random.default_rng(5000 + seed)
    rule = 1 if seed < 3 else 0
    K = None if cam is None else np.asarray(cam, np.float64)[:4]
    kw = {} if cam is None else dict(cam=cam)
    n_camera_edges = 0
    ctxs = {thr: pkg.VO(device=0, max_batch=1, pnp_reproj_thr=thr, **kw) for thr in thrs}
    for c_ in ctxs.values():
        c_.set_tuning(track_rule=rule)
    n_near = n_far_not_oldest = 0
    try:
        for case in range(10):
            thr = thrs[case % len(thrs)]; ctx = ctxs[thr]
            F = int(rng.integers(1, 40)); cap = int(rng.choice([64, 100, 256])); n_kf = int(rng.integers(1, 13))
            tables = list(_random_tracks(rng, F, cap, int(rng.integers(1, cap + 1))))
            tables[9] = _random_T_rel(rng, F, oracle)
            kf, ev, margin = _ref_keyframes(oracle, tables[9], n_kf)
            assert margin > 1e-9, (seed, case, margin)
            for b in range(1, F):
                if ev[b] >= 0:
                    n_near += int(np.linalg.norm(oracle.se3_log(oracle.se3_mul(_chain(oracle, tables[9])[ev[b]], oracle.se3_inv(_chain(oracle, tables[9])[b]))))
                                  < 0.2)
                    n_far_not_oldest += int(ev[b] != kf[b - 1][0])
            full = oracle.build_windows(*tables[:10], n_kf=max(F, 1), lm_capacity=F * cap * (F + 1), edge_capacity=2 * F * cap * (F + 1),
                                        reproj_thr=thr, track_rule=rule, K=K)
            if K is not None:
                kitti = oracle.build_windows(*tables[:10], n_kf=max(F, 1), lm_capacity=F * cap * (F + 1), edge_capacity=2 * F * cap * (F + 1),
                                             reproj_thr=thr, track_rule=rule)
                n_camera_edges += abs(int(full["edge_off"][F]) - int(kitti["edge_off"][F]))
            wins = _expected_windows(full, kf)
            nl_tot = sum(len(w) for w in wins); ne_tot = sum(sum(len(k) for k in w) for w in wins)
            shrink = rng.random() < 0.3 and nl_tot > 4
            lm_cap = max(int(nl_tot * rng.uniform(0.3, 0.9)), 1) if shrink else nl_tot + 7
            e_cap = ne_tot + 5
            g = _run(pkg, ctx, tables, n_kf, lm_cap, e_cap, use_nkps=case % 2 == 0)
            tag = (seed, case, F, cap, n_kf, shrink)
            assert np.array_equal(g["kf_frame"], kf) and np.array_equal(g["evicted"], ev), tag
            assert (g["st"][0] & 2) == 0, tag
            _compare(g, wins, kf, lm_cap, e_cap, _chain(oracle, tables[9]), tag)
        assert n_near > 0 and n_far_not_oldest > 0, (n_near, n_far_not_oldest)
    finally:
        for c_ in ctxs.values():
            c_.close()
    return n_camera_edges


def test_sliding_equivalence(pkg, oracle):
    """policy 0 is vslam_build_windows_dev bit for bit; so is policy 1 on a straight trajectory whose steps are >= 0.2 (the nearest frame is never
    close enough, the farthest is always the oldest)"""
    rng = np.random.default_rng(77)
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        for case in range(6):
            F = int(rng.integers(2, 40)); cap = int(rng.choice([64, 256])); n_kf = int(rng.integers(1, 13))
            tables = list(_random_tracks(rng, F, cap, int(rng.integers(1, cap + 1))))
            lm_cap, e_cap = F * cap * (n_kf + 1), 2 * F * cap * (n_kf + 1)
            if case >= 3:
                z = np.cumsum(np.concatenate([[0.0], rng.uniform(0.25, 1.5, F - 1)]))
                tables[9] = _z_steps(z)
            ref = _run(pkg, ctx, tables, n_kf, lm_cap, e_cap, legacy=True)
            for policy in ((0,) if case < 3 else (0, 1)):
                g = _run(pkg, ctx, tables, n_kf, lm_cap, e_cap, policy=policy)
                for k in ref:
                    if k not in ("kf_frame", "evicted"):
                        assert np.array_equal(g[k], ref[k]), (case, policy, k)
                b = np.arange(F)
                assert np.array_equal(g["evicted"], np.where(b >= n_kf, b - n_kf, -1)), (case, policy)
                for bb in range(F):
                    s = max(0, bb - n_kf + 1)
                    assert g["kf_frame"][bb].tolist() == list(range(s, bb + 1)) + [-1] * (n_kf - (bb + 1 - s)), (case, policy, bb)
    finally:
        ctx.close()


def _oracle_schedule(oracle, T, xyz, rel, kf, lm, uv):
    inl = np.ones(len(xyz), np.uint8)
    for iters, upd in ((5, False), (5, False), (10, True)):
        act = (inl.astype(bool) & rel)[lm]
        T2, _, chi2, _ = oracle.local_ba(T, xyz, kf[act], lm[act], uv[act], iters=iters)
        _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
        if upd:
            T = T2
    act = inl.astype(bool)[lm]
    T2, chi2, _ = oracle.pose_only_window(T, xyz, kf[act], lm[act], uv[act], iters=10)
    _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
    return T2, inl


def test_pipeline_reference_policy(oracle, synth):
    """rendered frames in ping-pong order (0..7, 6..0, 1..): the reversals put a frame next to an earlier one -- near-evictions on real tracks.
    The culled windows against the oracle restriction, the BA schedule on them against the oracle composite (slots need not be consecutive
    frames), and the trajectory against the per-frame gather"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 24, 10
    pipe = KeyframePipeline(B, anms_num=500, n_kf=n_kf, unique_frames=8, seed=6, ba_windows="tracks", window_policy="reference")
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        built = pipe.download()
        kf, ev, margin = _ref_keyframes(oracle, built["Tpnp"][:B - 1], n_kf)
        assert margin > 1e-9, margin
        assert np.array_equal(built["ba_kf_frame"], kf) and np.array_equal(built["ba_evicted"], ev)
        b = np.arange(B)
        assert (ev[b >= n_kf] != b[b >= n_kf] - n_kf).any(), "no step differs from the sliding window"
        full = oracle.build_windows(built["kps"][:B], built["lr"], built["nlr"], built["xyz"], built["valid"], built["rel"], built["f2f"][:B - 1],
                                    built["nf2f"][:B - 1], built["inl"][:B - 1], built["Tpnp"][:B - 1], n_kf=B)
        g = dict(lm_off=built["ba_lm_off"], e_off=built["ba_e_off"], nkf=built["ba_nkf"], T=built["ba_T"], xyz=built["ba_xyz"], rel=built["ba_rel"],
                 inl=built["ba_inl"], kf=built["ba_kf"], lm=built["ba_lm"], uv=built["ba_uv"], st=built["ba_build_status"])
        g["kf"] = g["kf"].copy(); g["kf"][g["e_off"][B]:] = -7   # (the pipeline's arrays are not pre-filled: nothing to check past the end)
        _compare(g, _expected_windows(full, kf), kf, pipe.lm_capacity, pipe.edge_capacity, _chain(oracle, built["Tpnp"][:B - 1]), "pipe",
                 xyz_tol=(2e-6, 1e-6))
        assert built["ba_build_status"][0] == 0
        # the BA schedule on culled windows
        pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        done = pipe.download()
        assert (pipe.vo.ba_status(B) == 0).all()
        lm_off, e_off = built["ba_lm_off"], built["ba_e_off"]
        culled = [w for w in range(B) if not np.array_equal(kf[w][kf[w] >= 0], np.arange(max(0, w - n_kf + 1), w + 1))]
        assert culled
        for w in sorted(set([0, 5] + culled[:2] + culled[-2:] + [B - 1])):
            nk = int(built["ba_nkf"][w])
            kfi, lmi, uvi = (built[k][e_off[w]:e_off[w + 1]] for k in ("ba_kf", "ba_lm", "ba_uv"))
            xyz = built["ba_xyz"][lm_off[w]:lm_off[w + 1]]; rel = built["ba_rel"][lm_off[w]:lm_off[w + 1]].astype(bool)
            T2, inl = _oracle_schedule(oracle, built["ba_T"][w][:nk].copy(), xyz, rel, kfi, lmi, uvi)
            assert np.allclose(done["ba_T"][w][:nk], T2, rtol=1e-4, atol=1e-6), (w, np.abs(done["ba_T"][w][:nk] - T2).max())
            got = done["ba_inl"][lm_off[w]:lm_off[w + 1]]
            assert np.array_equal(got, inl), (w, int((got != inl).sum()))
        # the trajectory: every frame once, each from the last window that held it
        ids, T = pipe.trajectory()
        assert sorted(ids.tolist()) == list(range(B)) and len(ids) == B
        for f, t in zip(ids, T):
            w = max(x for x in range(B) if f in kf[x])
            assert np.array_equal(t, done["ba_T"][w][int(np.flatnonzero(kf[w] == f)[0])]), f
    finally:
        pipe.close()


def test_refusals(pkg):
    """policy 1 on a chunk (the history before it decides which keyframes survive), a NaN or negative near_dist, an unknown policy, n_kf outside
    1..VSLAM_MAX_KF: VSLAM_ERR_ARG, nothing launched"""
    import torch
    rng = np.random.default_rng(3)
    tables = _random_tracks(rng, 6, 64, 40)
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
        g = _run(pkg, ctx, tables, 4, 4096, 8192)   # (valid: each case below differs in one argument)
        assert g["st"][0] == 0
        g = _run(pkg, ctx, tables, 4, 4096, 8192, policy=0, hook=chunk("d_T_abs"))   # (the sliding window on a chunk is fine)
        assert g["st"][0] == 0
        cases = [dict(near_dist=float("nan")), dict(near_dist=-0.1), dict(policy=2), dict(policy=-1), dict(n_kf_arg=0), dict(n_kf_arg=13)]
        cases += [dict(hook=chunk(m)) for m in ("d_T_abs", "d_carry_in", "d_carry_out")]
        for kw in cases:
            with pytest.raises(pkg.VslamError):
                _run(pkg, ctx, tables, 4, 4096, 8192, **kw)
    finally:
        ctx.close()
