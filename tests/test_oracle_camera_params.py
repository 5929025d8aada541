"""The oracle off the reference's camera and constants (CPU).

1. Axis exchange.  Every test of this suite used the KITTI camera, where fx == fy, so an fx in the place of an fy -- in a projection, a
   Jacobian, EPnP's normal equations, an inlier rule -- changed nothing.  Here the pose entries of the oracle run at cameras with fx != fy
   on a problem and on the same problem with x and y exchanged (tests/camera_variants.py: points (Y, X, Z), pixels (v, u), K (fy, fx, cy, cx),
   poses (S R S, S t)).  Code that treats the axes alike returns the exchanged answer; one mixed-up focal length breaks the identity grossly
   (the motion-only pose moves 0.3-0.5 m, inliers fall from 127 to 8).  No second implementation is trusted.
2. The constants the oracle used to hard-code (depth gates, matcher gate, FAST threshold) are arguments; each is checked against a few lines
   of numpy at values other than the reference's."""
import numpy as np
import pytest

import camera_variants as cv
from orb_restatements import fast_nms_numpy

CAMS = [pytest.param(cv.CAM_A, id="camA"), pytest.param(cv.CAM_B, id="camB")]
RTOL = 1e-4   # poses, landmarks, chi2 (the suite's parity tolerance); atol 1e-6 for poses and chi2, 1e-4 for landmarks


def _pose_close(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=1e-6)


def _pnp(synth, M, outl, seed, cam, **kw):
    return cv.recamera_problem(synth.pnp_problem(M=M, seed=seed, outlier_frac=outl, **kw), cam)


# ------------------------------------------------------------------ the helper itself
def test_recamera_and_swap_are_what_they_say(oracle, synth):
    p = synth.pnp_problem(M=50, seed=1, outlier_frac=0.0, sigma_px=0.0)
    K = cv.K4(cv.CAM_A)
    q = cv.recamera_problem(p, cv.CAM_A)
    uv, _ = synth.project(p["T_true"], p["xyz"].astype(np.float64), K)      # numpy projection with the new camera: the same pixels
    assert np.allclose(q["uv"], uv, atol=2e-3)                                # (f32 pixels, twice rounded)
    assert np.allclose(cv.recamera(p["uv"], cv.KITTI, cv.KITTI), p["uv"], rtol=0, atol=1e-4) and q["uv"].dtype == np.float32
    s, Ks = cv.swap_xy(q, K)
    assert list(Ks) == [820.0, 600.0, 260.5, 500.25]
    S = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1.0]])
    for key in ("T0", "T_true"):
        R = synth.R_from_quat(q[key][:4]); Rs = synth.R_from_quat(s[key][:4])
        assert np.allclose(Rs, S @ R @ S, atol=1e-14) and np.isclose(np.linalg.det(Rs), 1.0) and np.allclose(s[key][4:], S @ q[key][4:])
    uvs, _ = synth.project(s["T_true"], s["xyz"].astype(np.float64), Ks)
    assert np.allclose(uvs, uv[:, ::-1], atol=1e-9)
    assert np.array_equal(cv.swap_xy(s, Ks)[0]["uv"], q["uv"]) and np.allclose(cv.swap_xy(s, Ks)[0]["T0"], q["T0"])


# ------------------------------------------------------------------ residuals and Jacobians
@pytest.mark.parametrize("cam", CAMS)
def test_residuals_and_jacobians_under_exchange(oracle, synth, cam):
    rng = np.random.default_rng(7)
    K = cv.K4(cam); Ks = cv.swap_K(K)
    for _ in range(20):
        T = oracle.se3_exp(rng.normal(0, 0.3, 6)); pc = np.array([rng.normal(0, 2), rng.normal(0, 1), rng.uniform(8, 30)])
        pw = oracle.se3_act(oracle.se3_inv(T), pc); z = rng.uniform(0, 300, 2)
        e, Jp, Jl = oracle.projection_residual(T, pw, z, K)
        e1, J1 = oracle.pose_only_residual(T, pw, z, K)
        # the residual from the definition, with this camera's four numbers each in its place
        assert np.allclose(e, [z[0] - (K[0] * pc[0] / pc[2] + K[2]), z[1] - (K[1] * pc[1] / pc[2] + K[3])], rtol=1e-12, atol=1e-9)
        es, Jps, Jls = oracle.projection_residual(cv.swap_pose(T), cv.swap_points(pw), z[::-1].copy(), Ks)
        e1s, J1s = oracle.pose_only_residual(cv.swap_pose(T), cv.swap_points(pw), z[::-1].copy(), Ks)
        assert np.allclose(es, e[::-1], rtol=1e-10, atol=1e-9) and np.allclose(e1s, e1[::-1], rtol=1e-10, atol=1e-9)
        assert np.allclose(Jps, Jp[::-1][:, cv.POSE_COLS] * cv.POSE_SIGN, rtol=1e-9, atol=1e-9)
        assert np.allclose(J1s, J1[::-1][:, cv.POSE_COLS] * cv.POSE_SIGN, rtol=1e-9, atol=1e-9)
        assert np.allclose(Jls, Jl[::-1][:, cv.LM_COLS], rtol=1e-9, atol=1e-9)
        assert abs(Jp[0, 0]) != abs(Jp[1, 1])                                 # fx / Z against fy / Z: the two differ at these cameras


# ------------------------------------------------------------------ single-pose LM
@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("M,outl,seed", [(150, 0.15, 3), (500, 0.3, 4), (37, 0.0, 5)])
def test_pnp_motion_only_under_exchange(oracle, synth, cam, M, outl, seed):
    p = _pnp(synth, M, outl, seed, cam); K = cv.K4(cam)
    s, Ks = cv.swap_xy(p, K)
    T, inl, n, st = oracle.pnp_motion_only(p["xyz"], p["uv"], p["T0"], K)
    Ts, inls, ns, sts = oracle.pnp_motion_only(s["xyz"], s["uv"], s["T0"], Ks)
    assert n == ns and np.array_equal(inl, inls)
    assert _pose_close(Ts, cv.swap_pose(T)), np.abs(Ts - cv.swap_pose(T)).max()
    assert np.isclose(sts["chi2_final"], st["chi2_final"], rtol=RTOL, atol=1e-6) # (LM iteration counts may differ: once converged, round-off decides accept / reject)
    assert np.allclose(T, p["T_true"], atol=5e-2) and n >= 0.6 * M           # and it is the right answer at this camera


# ------------------------------------------------------------------ windows
@pytest.fixture(scope="module")
def window(synth):
    return synth.ba_window(n_kf=10, n_lm=300, seed=2)


@pytest.mark.parametrize("cam", CAMS)
def test_pose_only_window_under_exchange(oracle, window, cam):
    w = cv.recamera_problem(window, cam); K = cv.K4(cam)
    s, Ks = cv.swap_xy(w, K)
    T, chi2, st = oracle.pose_only_window(w["T0"], w["xyz"], w["kf_idx"], w["lm_idx"], w["uv"], K)
    Ts, chi2s, sts = oracle.pose_only_window(s["T0"], s["xyz"], s["kf_idx"], s["lm_idx"], s["uv"], Ks)
    assert _pose_close(Ts, cv.swap_pose(T))
    assert np.allclose(chi2s, chi2, rtol=RTOL, atol=1e-6)
    assert np.isclose(sts["chi2_final"], st["chi2_final"], rtol=RTOL)
    assert np.abs(T - w["T0"]).max() > 1e-3 and np.allclose(T, w["T_true"], atol=5e-2)


@pytest.mark.parametrize("cam", CAMS)
def test_local_ba_under_exchange(oracle, window, cam):
    w = cv.recamera_problem(window, cam); K = cv.K4(cam)
    s, Ks = cv.swap_xy(w, K)
    T, xyz, chi2, st = oracle.local_ba(w["T0"], w["xyz"], w["kf_idx"], w["lm_idx"], w["uv"], K, update_poses=True, update_lms=True)
    Ts, xyzs, chi2s, sts = oracle.local_ba(s["T0"], s["xyz"], s["kf_idx"], s["lm_idx"], s["uv"], Ks, update_poses=True, update_lms=True)
    assert _pose_close(Ts, cv.swap_pose(T))
    assert np.allclose(xyzs, cv.swap_points(xyz), rtol=RTOL, atol=1e-4)
    assert np.allclose(chi2s, chi2, rtol=RTOL, atol=1e-6)
    assert np.isclose(sts["chi2_final"], st["chi2_final"], rtol=RTOL)
    assert np.abs(xyz - w["xyz"]).max() > 1e-2 and st["chi2_final"] < 0.5 * st["chi2_init"]


# ------------------------------------------------------------------ RANSAC over EPnP
# The inliers of these problems are exact (sigma_px = 0; outliers stay gross).  EPnP refines its betas with FIVE Gauss-Newton iterations from
# start values that depend on the basis its eigen-solver returns for the (two-dimensional, for 5 points) null space of M^T M (oracle/epnp.c,
# header) -- and the exchange permutes M^T M, so that basis changes.  On exact correspondences the start values already solve the six distance
# equations and the model is a function of the geometry alone: the identity holds to round-off (measured: <= 9e-7 over 13 problems x 2 cameras
# x 6 settings, typically 1e-13).  On noisy 5-point subsets the five iterations do not always converge and the returned hypothesis differs by
# 1e-5 .. 1e-2 in 7 of 156 settings at lm_iters = 0 (masks equal in 154); with 60 iterations in a scratch copy of epnp.c those differences
# drop to 1e-13, so they are the fixed iteration count and not a focal length in the wrong place.  A mixed-up fx / fy moves poses by 0.3-0.5 m
# on exact data as on noisy data.
RANSAC_PROBLEMS = [(400, 0.35, 9), (80, 0.2, 1), (6, 0.0, 4), (5, 0.0, 5), (150, 0.15, 3), (1500, 0.3, 2)]


@pytest.mark.parametrize("cam", CAMS)
@pytest.mark.parametrize("M,outl,seed", RANSAC_PROBLEMS)
def test_pnp_ransac_under_exchange(oracle, synth, cam, M, outl, seed):
    p = _pnp(synth, M, outl, seed, cam, sigma_px=0.0); K = cv.K4(cam)
    s, Ks = cv.swap_xy(p, K)
    for lm_iters in (0, 10):
        for err in (1.5, 4.0, 8.0):
            T, inl, n, it = oracle.pnp_ransac(p["xyz"], p["uv"], K=K, reproj_err=err, lm_iters=lm_iters)
            Ts, inls, ns, its = oracle.pnp_ransac(s["xyz"], s["uv"], K=Ks, reproj_err=err, lm_iters=lm_iters)
            assert (n, it) == (ns, its) and np.array_equal(inl, inls), (lm_iters, err, n, ns, it, its)
            assert _pose_close(Ts, cv.swap_pose(T)), (lm_iters, err, np.abs(Ts - cv.swap_pose(T)).max())
            assert inl[~p["outlier"]].all() and np.allclose(T, p["T_true"], atol=5e-2)   # and it is the right answer


@pytest.mark.parametrize("cam", CAMS)
def test_epnp_subsets_under_exchange(oracle, synth, cam):
    """every 5-point EPnP model of the hypothesis sequence, and its inlier count under the f32 error rule"""
    p = _pnp(synth, 257, 0.0, 1, cam, sigma_px=0.0); K = cv.K4(cam)
    s, Ks = cv.swap_xy(p, K)
    subs = oracle.ransac_subsets(257, 100)
    R_true = synth.R_from_quat(p["T_true"][:4])
    for h in range(100):
        m = oracle.epnp_subset(p["xyz"], p["uv"], subs[h], K); ms = oracle.epnp_subset(s["xyz"], s["uv"], subs[h], Ks)
        assert m is not None and ms is not None
        assert np.allclose(ms, cv.swap_model(m), rtol=RTOL, atol=1e-6), (h, np.abs(ms - cv.swap_model(m)).max())
        assert np.allclose(m[:9].reshape(3, 3), R_true, atol=1e-3) and np.allclose(m[9:], p["T_true"][4:], atol=2e-2), h
        for err in (1.5, 4.0, 8.0):
            c = oracle.pnp_ransac_hypothesis(p["xyz"], p["uv"], h, K, err)[1]
            assert c == oracle.pnp_ransac_hypothesis(s["xyz"], s["uv"], h, Ks, err)[1] and c >= 5


# ------------------------------------------------------------------ the constants that became arguments
def _camera_depth(xyz_w, T):
    R = np.array([[1 - 2 * (T[1] ** 2 + T[2] ** 2), 2 * (T[0] * T[1] - T[2] * T[3]), 2 * (T[0] * T[2] + T[1] * T[3])],
                  [2 * (T[0] * T[1] + T[2] * T[3]), 1 - 2 * (T[0] ** 2 + T[2] ** 2), 2 * (T[1] * T[2] - T[0] * T[3])],
                  [2 * (T[0] * T[2] - T[1] * T[3]), 2 * (T[1] * T[2] + T[0] * T[3]), 1 - 2 * (T[0] ** 2 + T[1] ** 2)]])
    with np.errstate(invalid="ignore", over="ignore"):
        return (xyz_w.astype(np.float64) @ R.T + T[4:])[:, 2]


def _check_gates(xyz, valid, rel, T, gate):
    """valid = min < Z < max, reliable = valid and Z < reliable, on the camera-frame depth of the oracle's own world point; a point whose
    depth is within f32 rounding of a gate (the stored point is f32) is left out"""
    Z = _camera_depth(xyz, T)
    with np.errstate(invalid="ignore"):
        near = np.zeros(len(Z), bool)
        for g in gate:
            near |= np.abs(Z - g) <= 1e-5 * g
        want_v = (Z > gate[0]) & (Z < gate[1]); want_r = want_v & (Z < gate[2])
    assert near.sum() <= 0.01 * len(Z)
    assert np.array_equal(valid[~near].astype(bool), want_v[~near]) and np.array_equal(rel[~near].astype(bool), want_r[~near])
    return int(want_v.sum()), int(want_r.sum())


@pytest.mark.parametrize("cam", CAMS + [pytest.param(cv.KITTI, id="kitti")])
@pytest.mark.parametrize("gate", [(10.0, 400.0, 40.0), (3.0, 150.0, 25.0)])
def test_depth_gates_are_arguments(oracle, cam, gate):
    uvL, uvR, T = cv.stereo_pixels(cam)
    x0, v0, r0 = oracle.triangulate_dlt(uvL, uvR, T, cam, row_tol=-1)
    x, v, r = oracle.triangulate_dlt(uvL, uvR, T, cam, row_tol=-1, depth_gate=gate)
    assert np.array_equal(x.view(np.uint32), x0.view(np.uint32))               # the gate only flags
    nv, nr = _check_gates(x, v, r, T, gate)
    assert 50 < nr < nv < len(x) - 100
    if gate != oracle.DEPTH_GATE:
        assert (v != v0).sum() > 20 and (r != r0).sum() > 20
    # the disparity-map entry applies the same rule
    rng = np.random.default_rng(1)
    disp = rng.uniform(0.5, 90, (120, 400)).astype(np.float32)
    disp[rng.random(disp.shape) < 0.1] = -1.0; disp[rng.random(disp.shape) < 0.02] = 0.0
    kps = np.zeros(1500, oracle.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(0, 399, len(kps)); kps["y"] = rng.uniform(0, 119, len(kps))
    x, v, r = oracle.find_3d_disparity(kps, disp, T, cam, depth_gate=gate)
    fin = np.isfinite(x).all(1)
    nv, nr = _check_gates(x[fin], v[fin], r[fin], T, gate)
    assert not v[~fin].any() and nv > 50 and nr >= 0
    # and the depth is fx b / d with THIS camera's fx and b, x and y scaled by its own fx, fy
    d = disp[kps["y"].astype(int), kps["x"].astype(int)].astype(np.float64)
    ok = v.astype(bool)
    Zc = cam[0] * cam[4] / d[ok]
    pc = np.stack([(kps["x"][ok].astype(np.float64) - cam[2]) / cam[0] * Zc, (kps["y"][ok].astype(np.float64) - cam[3]) / cam[1] * Zc, Zc], 1)
    Ti = oracle.se3_inv(T)
    want = pc @ oracle.se3_rotmat(Ti).T + Ti[4:]
    assert np.allclose(x[ok], want, rtol=1e-5, atol=1e-5)


def test_triangulate_exact_at_cameras_with_unequal_focal_lengths(oracle):
    """consistent stereo pixels of camera A / B triangulate back to the points that made them (an fx in the place of an fy would not)"""
    rng = np.random.default_rng(3)
    for cam in (cv.CAM_A, cv.CAM_B):
        fx, fy, cx, cy, b = cam
        P = np.stack([rng.uniform(-6, 6, 400), rng.uniform(-3, 3, 400), rng.uniform(11, 39, 400)], 1)
        uvL = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1)
        uvR = np.stack([fx * (P[:, 0] - b) / P[:, 2] + cx, uvL[:, 1]], 1)
        T = oracle.se3_exp(rng.normal(0, 0.2, 6)); Ti = oracle.se3_inv(T)
        xyz, valid, rel = oracle.triangulate_dlt(uvL, uvR, T, cam)
        assert valid.all() and rel.all()
        assert np.allclose(xyz, P @ oracle.se3_rotmat(Ti).T + Ti[4:], rtol=5e-3, atol=5e-2)   # f32 pixels: depth error ~ Z^2 / (fx b) * 2^-15 px


@pytest.mark.parametrize("row_tol", [0.25, 2.0, -1.0])
def test_row_tolerance_is_an_argument(oracle, row_tol):
    uvL, uvR, T = cv.stereo_pixels(cv.CAM_A)
    x, v, r = oracle.triangulate_dlt(uvL, uvR, T, cv.CAM_A, row_tol=row_tol)
    xo, vo_, ro = oracle.triangulate_dlt(uvL, uvR, T, cv.CAM_A, row_tol=-1)
    rows_ok = (np.abs(uvL[:, 1].astype(np.float64) - uvR[:, 1].astype(np.float64)) <= row_tol) & (uvL[:, 0] > uvR[:, 0]) if row_tol >= 0 else np.ones(len(v), bool)
    assert np.array_equal(v.astype(bool), vo_.astype(bool) & rows_ok) and np.array_equal(r.astype(bool), ro.astype(bool) & rows_ok)
    assert 0 < v.sum() and (row_tol != 0.25 or v.sum() < 0.7 * vo_.sum())


@pytest.mark.parametrize("ratio,gap_thr", [(2.0, 30.0), (1.2, 10.0), (3.0, 60.0)])
def test_matcher_gate_is_an_argument(oracle, synth, ratio, gap_thr):
    q, t = synth.random_descriptors(300, 300, seed=5, flip_p=0.1)
    raw = oracle.bf_match_xcheck(q, t)
    counts = []
    for gap in (1.0, 2.0):
        thr = max(ratio * float(raw["distance"].min()), gap_thr * gap)
        want = raw[raw["distance"].astype(np.float64) <= thr]
        got = oracle.feature_matching(q, t, gap, ratio=ratio, gap_thr=gap_thr)
        assert np.array_equal(got, want)
        counts.append(len(got))
    if (ratio, gap_thr) == (2.0, 30.0):
        assert np.array_equal(oracle.feature_matching(q, t, 1.0), oracle.feature_matching(q, t, 1.0, ratio=2.0, gap_thr=30.0))
    else:
        assert counts[0] != len(oracle.feature_matching(q, t, 1.0))
    assert 0 < counts[0] <= counts[1] <= len(raw)


@pytest.mark.parametrize("thr", [7, 20, 40])
def test_fast_threshold_is_an_argument(oracle, synth, thr):
    """orb_detect at a FAST threshold other than 20: with a feature budget nothing is culled by, level 0 is exactly the non-max-suppressed
    FAST-9/16 corner set of that threshold (numpy restatement) inside the 31 px border, in raster order"""
    img = synth.noise_image(5, 320, 200)
    kps = oracle.orb_detect(img, nfeatures=200000, cap=65536, fast_threshold=thr)
    k0 = kps[kps["octave"] == 0]
    keep, score = fast_nms_numpy(img, thr)
    keep[:31] = False; keep[-31:] = False; keep[:, :31] = False; keep[:, -31:] = False
    ys, xs = np.nonzero(keep)
    assert np.array_equal(k0["x"], xs.astype(np.float32)) and np.array_equal(k0["y"], ys.astype(np.float32))
    base = oracle.orb_detect(img, nfeatures=200000, cap=65536)
    if thr == 20:
        assert np.array_equal(kps, base)
    else:
        assert (len(kps) > 1.5 * len(base)) if thr < 20 else (0 < len(kps) < 0.7 * len(base))
    # feature_detection passes the threshold on: detect(thr) -> ANMS -> compute
    fk, fd = oracle.feature_detection(img, nfeatures=1000, anms_num=200, fast_threshold=thr)
    d = oracle.orb_detect(img, nfeatures=1000, fast_threshold=thr)
    wk, wd = oracle.orb_compute(img, oracle.anms(d, 200))
    assert np.array_equal(fk, wk) and np.array_equal(fd, wd) and len(fk) > 0


@pytest.mark.parametrize("thr0", [1.5, 5.991, 40.0])
def test_chi2_threshold_starts_at_the_huber_width(oracle, window, thr0):
    """optimization.cpp:154 / :205: `chi2_th` is one variable, the Huber delta and the first classification threshold; the oracle takes it as an
    argument (default 5.991) and doubles it up to five times while half of the edges or more lie above it"""
    w = cv.recamera_problem(window, cv.CAM_A)
    _, _, chi2, _ = oracle.local_ba(w["T0"], w["xyz"], w["kf_idx"], w["lm_idx"], w["uv"], cv.K4(cv.CAM_A), 3, thr0)
    th, inl, ni, no = oracle.chi2_classify(chi2, w["lm_idx"], np.ones(len(w["xyz"]), np.uint8), thr0)
    want = thr0
    for _ in range(5):
        if (chi2 <= want).mean() > 0.5:
            break
        want *= 2
    assert th == want and ni == int((chi2 <= want).sum()) and ni + no == len(chi2)
    last = {int(l): e for e, l in enumerate(w["lm_idx"])}
    assert all(inl[l] == (chi2[e] <= want) for l, e in last.items())
    if thr0 == 5.991:
        assert th == oracle.chi2_classify(chi2, w["lm_idx"], np.ones(len(w["xyz"]), np.uint8))[0]
    else:
        assert not np.array_equal(inl, oracle.chi2_classify(chi2, w["lm_idx"], np.ones(len(w["xyz"]), np.uint8))[1])


def test_cpu_shim_honours_every_params_field(oracle, pkg, synth, window):
    """libvslam_cpu_shim.so (the host tier of the C-ABI served by the oracle) passes the context's depth gates, matcher gate and FAST
    threshold through instead of refusing them"""
    import ctypes as C
    import os
    so = os.path.join(os.path.dirname(os.path.abspath(oracle.__file__)), "libvslam_cpu_shim.so")
    lib = C.CDLL(so)
    P = pkg.Params()
    lib.vslam_default_params(C.byref(P))
    P.fast_threshold = 40; P.depth_min, P.depth_max, P.depth_reliable = 3.0, 150.0, 25.0
    P.match_ratio, P.match_gap_thr = 1.2, 10.0; P.stereo_row_tol = 0.25; P.huber_delta = 1.5
    for i in range(5):
        P.cam[i] = cv.CAM_A[i]
    h = C.c_void_p()
    assert lib.vslam_create(C.byref(P), 0, None, C.byref(h)) == 0
    try:
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        uvL, uvR, T = cv.stereo_pixels(cv.CAM_A)
        n = len(uvL)
        xyz = np.zeros((n, 3), np.float32); valid = np.zeros(n, np.uint8); rel = np.zeros(n, np.uint8); nv = C.c_int()
        assert lib.vslam_triangulate(h, vp(uvL), vp(uvR), n, vp(T), vp(xyz), vp(valid), vp(rel), C.byref(nv)) == 0
        wx, wv, wr = oracle.triangulate_dlt(uvL, uvR, T, cv.CAM_A, row_tol=0.25, depth_gate=(3.0, 150.0, 25.0))
        assert np.array_equal(valid, wv) and np.array_equal(rel, wr) and np.array_equal(xyz, wx) and nv.value == wv.sum()
        assert not np.array_equal(wv, oracle.triangulate_dlt(uvL, uvR, T, cv.CAM_A, row_tol=0.25)[1])
        q, t = synth.random_descriptors(137, 211, seed=3, flip_p=0.1)
        out = np.zeros(len(q), oracle.DMATCH_DTYPE); nm = C.c_int()
        assert lib.vslam_feature_matching(h, vp(q), len(q), vp(t), len(t), C.c_double(1.0), 1, vp(out), C.byref(nm)) == 0
        want = oracle.feature_matching(q, t, 1.0, ratio=1.2, gap_thr=10.0)
        assert np.array_equal(out[:nm.value], want) and len(want) != len(oracle.feature_matching(q, t, 1.0))
        img = synth.noise_image(5, 320, 200)
        cap = 4096
        kps = np.zeros(cap, oracle.KEYPOINT_DTYPE); desc = np.zeros((cap, 32), np.uint8); nk = C.c_int()
        assert lib.vslam_feature_detection(h, vp(img), 320, 200, 320, vp(kps), vp(desc), cap, C.byref(nk)) == 0
        wk, wd = oracle.feature_detection(img, fast_threshold=40)
        assert np.array_equal(kps[:nk.value], wk) and np.array_equal(desc[:nk.value], wd)
        assert len(wk) != len(oracle.feature_detection(img)[0])
        # optimize_map: the Huber width, which is also where the chi2 classification starts
        w = cv.recamera_problem(window, cv.CAM_A)
        T = w["T0"].copy(); xyz = w["xyz"].copy(); n_lm = len(xyz); ne = len(w["kf_idx"])
        inl = np.ones(n_lm, np.uint8); chi2 = np.zeros(ne); thr = C.c_double()
        assert lib.vslam_local_ba(h, len(T), vp(T), n_lm, vp(xyz), ne, vp(w["kf_idx"]), vp(w["lm_idx"]), vp(w["uv"]), None, None, 5, 1, 1, vp(inl), vp(chi2),
                                  C.byref(thr), None) == 0
        wT, wxyz, wchi2, _ = oracle.local_ba(w["T0"], w["xyz"], w["kf_idx"], w["lm_idx"], w["uv"], cv.K4(cv.CAM_A), 5, 1.5, True, True)
        wth, winl, _, _ = oracle.chi2_classify(wchi2, w["lm_idx"], np.ones(n_lm, np.uint8), 1.5)
        assert np.array_equal(T, wT) and np.array_equal(xyz, wxyz) and np.array_equal(chi2, wchi2) and thr.value == wth and np.array_equal(inl, winl)
        assert wth != oracle.chi2_classify(wchi2, w["lm_idx"], np.ones(n_lm, np.uint8))[0]
    finally:
        lib.vslam_destroy(h)
