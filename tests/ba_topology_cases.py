"""BA windows whose GRAPH is unusual -- a keyframe without edges, two keyframe groups that share no landmark, only single-observation landmarks, every
landmark seen by every keyframe, landmark counts on and around the 64-landmark row, edge counts around 256, unobserved landmarks between observed
ones, one edge, no edge -- and are otherwise well conditioned: the inputs of tests/test_ba_topology_cases.py (CPU guards) and
tests/test_gpu_ba_topology.py (the BA kernels against the oracle and against recompute_chi2 below).

A case is a dict with T0 (n_kf, 7) f64, xyz (n_lm, 3) f32, kf_idx / lm_idx (n_edge,) i32 sorted by landmark, uv (n_edge, 2) f32, n_kf, name, and
optionally inl0 (n_lm,) u8: landmarks handed in as outliers.  Where a construction drops edges, landmarks left without an edge are dropped too and the
rest re-numbered (lm_idx < n_lm), except where the case is about keeping them.

recompute_chi2 imports nothing from oracle/: it is written from the edge definition of the reference (optimization.cpp:41-50, EdgeProjection::
computeError: pos_pixel = K (T p), divided by its third component, error = measurement - pixel)."""
import numpy as np

from stereo_visual_slam_amd import synth

K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157])   # types_def.hpp:53-54
HUBER_DELTA = 5.991                                          # optimization.cpp:154, :205: the chi2 threshold, handed to the Huber kernel as its delta
CHI2_TH0 = 5.991

# the seed of every case: the oracle alone meets guards B and C of tests/test_ba_topology_cases.py at it (a case that does not gets the next seed; none needed one)
SEEDS = dict(kf_first_empty=5, kf_mid_empty=5, kf_last_empty=5, kf_one_edge=5, kf_two_edges=5, disconnected=5, all_singles=5, all_see_all=5,
             rows_63=5, rows_64=5, rows_65=5, rows_129=5, edges_255=5, edges_256=5, edges_257=5, unobserved_interleaved=5, one_edge=5,
             zero_edges=5, all_outliers_in=5, behind_camera=5, normal_a=905, normal_b=906)
EMPTY_KF = dict(kf_first_empty=0, kf_mid_empty=3, kf_last_empty=5)   # the keyframe without an edge
HOST_ONLY_SKIP = ("all_outliers_in",)                               # for the batched schedule only: the host entries take no flags in
NO_TRAJECTORY = ("zero_edges", "one_edge")                           # exempt from guard B


def _cut(w, keep, n_kf=None, drop_unobserved=True, name=None):
    """the window with the edges keep (bool per edge); landmarks without an edge dropped and the others re-numbered unless drop_unobserved is off"""
    kf, lm, uv = w["kf_idx"][keep], w["lm_idx"][keep], w["uv"][keep]
    xyz = w["xyz"]
    if drop_unobserved:
        seen = np.zeros(len(xyz), bool)
        seen[lm] = True
        new_id = np.cumsum(seen) - 1
        lm = new_id[lm]; xyz = xyz[seen]
    n_kf = len(w["T0"]) if n_kf is None else n_kf
    return dict(name=name, T0=np.ascontiguousarray(w["T0"][:n_kf], np.float64), xyz=np.ascontiguousarray(xyz, np.float32), kf_idx=np.ascontiguousarray(kf, np.int32),
                lm_idx=np.ascontiguousarray(lm, np.int32), uv=np.ascontiguousarray(uv, np.float32), n_kf=n_kf)


def _base(seed, n_kf=6, n_lm=150, min_obs=1, max_obs=4):
    return synth.ba_window(n_kf=n_kf, n_lm=n_lm, min_obs=min_obs, max_obs=max_obs, seed=seed)


def _quat_rotate(q, p):
    """p rotated by the unit quaternion q = (x, y, z, w): p + 2 w (v x p) + 2 v x (v x p)"""
    v, w = q[..., :3], q[..., 3:4]
    c = np.cross(v, p)
    return p + 2.0 * (w * c + np.cross(v, c))


def _quat_rotate_inv(q, p):
    return _quat_rotate(np.concatenate([-q[..., :3], q[..., 3:4]], -1), p)


def make_case(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    every = lambda w: np.ones(len(w["kf_idx"]), bool)
    if name in EMPTY_KF:
        w = _base(seed)
        return _cut(w, w["kf_idx"] != EMPTY_KF[name], name=name)
    if name in ("kf_one_edge", "kf_two_edges"):
        w = _base(seed)
        on3 = np.flatnonzero(w["kf_idx"] == 3)
        keep = w["kf_idx"] != 3
        keep[on3[:1 if name == "kf_one_edge" else 2]] = True
        return _cut(w, keep, name=name)
    if name == "disconnected":
        w = _base(seed)
        first = np.full(len(w["xyz"]), -1)
        for e in range(len(w["kf_idx"]) - 1, -1, -1):
            first[w["lm_idx"][e]] = w["kf_idx"][e]                   # (descending: the first edge of a landmark is written last)
        return _cut(w, (w["kf_idx"] < 3) == (first[w["lm_idx"]] < 3), name=name)
    if name == "all_singles":
        w = _base(seed, min_obs=1, max_obs=1)
        return _cut(w, every(w), name=name)
    if name == "all_see_all":
        w = _base(seed, n_kf=12, n_lm=40, min_obs=12, max_obs=12)
        return _cut(w, every(w), name=name)
    if name.startswith("rows_"):
        w = _base(seed, n_lm=int(name[5:]), min_obs=2, max_obs=4)
        return _cut(w, every(w), name=name)
    if name.startswith("edges_"):
        w = _base(seed)
        return _cut(w, np.arange(len(w["kf_idx"])) < int(name[6:]), name=name)
    if name == "unobserved_interleaved":
        w = _base(seed)
        return _cut(w, w["lm_idx"] % 5 != 2, drop_unobserved=False, name=name)
    if name == "one_edge":
        w = _base(seed, n_kf=1, n_lm=1, min_obs=1, max_obs=1)
        return _cut(w, every(w), name=name)
    if name == "zero_edges":
        w = _base(seed, n_lm=20)
        return _cut(w, ~every(w), drop_unobserved=False, name=name)
    if name == "all_outliers_in":
        c = _cut(_base(seed), every(_base(seed)), name=name)
        c["inl0"] = np.zeros(len(c["xyz"]), np.uint8)
        return c
    if name == "behind_camera":
        w = _base(seed)
        c = _cut(w, every(w), name=name)
        cnt = np.bincount(c["lm_idx"], minlength=len(c["xyz"]))
        l = int(np.flatnonzero(cnt >= 2)[len(np.flatnonzero(cnt >= 2)) // 2])   # a multi-observation landmark from the middle of the id range
        k = int(c["kf_idx"][np.flatnonzero(c["lm_idx"] == l)[0]])
        q, t = c["T0"][k, :4], c["T0"][k, 4:]
        pc = _quat_rotate(q, c["xyz"][l].astype(np.float64)) + t
        pc[2] = -5.0
        c["xyz"][l] = _quat_rotate_inv(q, pc - t).astype(np.float32)
        c["moved"] = (l, k)
        return c
    if name in ("normal_a", "normal_b"):   # the windows around the cases in the batched schedule: synth.ba_window_fast as the other batch tests use it
        w = synth.ba_window_fast(n_kf=10, n_lm=300, seed=seed)
        return _cut(w, every(w), name=name)
    raise KeyError(name)


def case_names():
    """the cases proper, without the two ordinary windows that frame them in the batched schedule"""
    return [k for k in SEEDS if not k.startswith("normal_")]


_cache = {}


def cases():
    """{name: case}, built once per process; callers must not write into the arrays"""
    if not _cache:
        for n in SEEDS:
            _cache[n] = make_case(n)
            for k in ("T0", "xyz", "kf_idx", "lm_idx", "uv"):
                _cache[n][k].setflags(write=False)
    return _cache


def oracle_schedule(oracle, case, trace=None):
    """the composite schedule of run_vslam.cpp:58-71 on one window, starting from the case's inl0: optimize_map(5), optimize_map(5) without write-back,
    optimize_map(10) writing the poses, every one followed by the chi2 classification over the edges of the landmarks still flagged in, then
    optimize_pose_only(10) and its classification.  Returns (T, lm_inlier); trace, a list, receives (chi2, threshold, flag landmark per edge) of
    every classification."""
    T, xyz, kf, lm, uv = case["T0"].copy(), case["xyz"], case["kf_idx"], case["lm_idx"], case["uv"]
    inl = case["inl0"].copy() if case.get("inl0") is not None else np.ones(len(xyz), np.uint8)
    for iters, upd in ((5, False), (5, False), (10, True)):
        act = inl.astype(bool)[lm]
        T2, _, chi2, _ = oracle.local_ba(T, xyz, kf[act], lm[act], uv[act], iters=iters)
        th, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
        if trace is not None:
            trace.append((chi2, th, lm[act]))
        if upd:
            T = T2
    act = inl.astype(bool)[lm]
    T2, chi2, _ = oracle.pose_only_window(T, xyz, kf[act], lm[act], uv[act], iters=10)
    th, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
    if trace is not None:
        trace.append((chi2, th, lm[act]))
    return T2, inl


def _camera_points(T, xyz, kf_idx, lm_idx):
    T = np.asarray(T, np.float64).reshape(-1, 7); p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    kf_idx = np.asarray(kf_idx, np.int64); lm_idx = np.asarray(lm_idx, np.int64)
    return _quat_rotate(T[kf_idx, :4], p[lm_idx]) + T[kf_idx, 4:]


def residuals(T, xyz, kf_idx, lm_idx, uv, K=K_KITTI):
    """(n_edge, 2) f64: measurement - K (T p) / (K (T p))[2], the reference's order of operations"""
    pc = _camera_points(T, xyz, kf_idx, lm_idx)
    px = K[0] * pc[:, 0] + K[2] * pc[:, 2]; py = K[1] * pc[:, 1] + K[3] * pc[:, 2]
    z = np.asarray(uv).astype(np.float64).reshape(-1, 2)
    return np.stack([z[:, 0] - px / pc[:, 2], z[:, 1] - py / pc[:, 2]], 1)


def huber_sum(chi2, delta=HUBER_DELTA):
    """g2o RobustKernelHuber on e = chi2: e below delta^2, 2 sqrt(e) delta - delta^2 above"""
    chi2 = np.asarray(chi2, np.float64)
    return float(np.where(chi2 <= delta * delta, chi2, 2.0 * np.sqrt(chi2) * delta - delta * delta).sum())


def recompute_chi2(T, xyz, kf_idx, lm_idx, uv, K=K_KITTI):
    """(per-edge e . e, Huber-robust sum with delta^2 = 5.991^2 as the reference sets it) of the state (T, xyz), plain numpy f64"""
    e = residuals(T, xyz, kf_idx, lm_idx, uv, K)
    chi2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    return chi2, huber_sum(chi2)


def f32_storage_allowance(T, xyz, kf_idx, lm_idx, uv, K=K_KITTI):
    """How far the chi2 of an edge can move when its landmark, kept in f64 by the optimiser, is stored as f32: every coordinate moves by at most half an
    f32 ulp of the landmark's largest coordinate, h = ulp_f32(max |xyz_l|) / 2, so e moves by at most d_i = sum_j |de_i/dp_j| h per component and
    chi2 = e . e by at most 2 sum_i |e_i| d_i + sum_i d_i^2 (the second term matters only where e is almost zero), plus 1e-9 chi2 for the two f64
    evaluations.  de/dp = -[[fx/Z, 0, -fx X/Z^2], [0, fy/Z, -fy Y/Z^2]] R (optimization.cpp:68-72)."""
    pc = _camera_points(T, xyz, kf_idx, lm_idx)
    X, Y, Z = pc[:, 0], pc[:, 1], pc[:, 2]
    T = np.asarray(T, np.float64).reshape(-1, 7)
    q = T[np.asarray(kf_idx, np.int64), :4]
    R = np.stack([_quat_rotate(q, np.broadcast_to(ax, (len(q), 3))) for ax in np.eye(3)], 2)   # (n, 3, 3): column j = R e_j
    Jc = np.zeros((len(q), 2, 3))
    Jc[:, 0, 0] = -K[0] / Z; Jc[:, 0, 2] = K[0] * X / (Z * Z); Jc[:, 1, 1] = -K[1] / Z; Jc[:, 1, 2] = K[1] * Y / (Z * Z)
    J = Jc @ R
    p32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    h = 0.5 * np.spacing(np.abs(p32).max(1)).astype(np.float64)[np.asarray(lm_idx, np.int64)]
    d = np.abs(J).sum(2) * h[:, None]
    e = residuals(T, xyz, kf_idx, lm_idx, uv, K)
    return 2.0 * (np.abs(e) * d).sum(1) + (d * d).sum(1) + 1e-9 * (e * e).sum(1)


def chi2_floor(uv):
    """A cost below which two correct f64 evaluations of the same window differ by more than they agree: a residual component is a pixel-sized
    quantity that went through at least eight roundings (rotate, translate, scale by the focal length, add the principal point, divide, subtract),
    d = 8 * 2^-53 * max |uv|, and the cost of n_edge edges cannot be told from zero below n_edge * 2 d^2 (about 1e-24 px^2 per edge)."""
    uv = np.asarray(uv, np.float64)
    if uv.size == 0:
        return 0.0
    d = 8.0 * 2.0 ** -53 * float(np.abs(uv).max())
    return len(uv.reshape(-1, 2)) * 2.0 * d * d


def significant_prefix(st):
    """iterations whose chi2 decrease is numerically significant, as tests/test_gpu_lm.py::_stats_close counts them on the oracle's record"""
    prev = st["chi2_init"]; sig = 0
    for i, c in enumerate(st["chi2_iter"]):
        if (prev - c) <= 1e-7 * prev:
            break
        prev = c; sig = i + 1
    return sig


def last_accepted_iteration(st):
    """The optimiser (g2o's, the oracle's, the kernels') leaves the per-edge chi2 of the last TRIAL it evaluated; the state it returns is the last
    ACCEPTED one.  The two coincide when the last iteration ended in an accepted trial, i.e. when it changed the chi2 record.  Returns the number of
    leading iterations after which they coincide (the 1-based index of the last iteration that changed chi2; 0: none did)."""
    prev = st["chi2_init"]; last = 0
    for i, c in enumerate(st["chi2_iter"]):
        if c != prev:
            last = i + 1
        prev = c
    return last


def deciding_edges(flag_lm, n_lm):
    """the edge that decides each landmark's flag: the last one in edge order (optimization.cpp:254-266 overwrites per edge)"""
    last = np.full(n_lm, -1)
    last[np.asarray(flag_lm)] = np.arange(len(flag_lm))
    return last[last >= 0]
