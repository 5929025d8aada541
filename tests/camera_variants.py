"""Cameras with fx != fy and the two input transformations the camera-parameter tests are built on (plain numpy, no GPU).

Every synthetic generator of stereo_visual_slam_amd/synth.py uses the KITTI camera, where fx == fy: an fx in the place of an fy is invisible
there.  `recamera` turns a generator's output into a problem for another camera without touching its geometry; `swap_xy` exchanges the
x and y axes of a whole problem.  An implementation that treats the two axes alike returns, for the exchanged problem, the exchanged
answer -- an identity that needs no trusted second implementation (tests/test_oracle_camera_params.py)."""
import numpy as np

KITTI = (718.856, 718.856, 607.1928, 185.2157, 0.573)   # fx, fy, cx, cy, baseline (types_def.hpp:53-54)
CAM_A = (600.0, 820.0, 500.25, 260.5, 0.31)
CAM_B = (1200.5, 900.25, 300.0, 100.0, 0.12)

_POSE_KEYS = ("T0", "T_true")


def K4(cam):
    return np.asarray(cam, np.float64)[:4].copy()


def recamera(uv, K_from, K_to):
    """the pixels of the same viewing rays in another camera: u' = (u - cx) / fx * fx' + cx', likewise v; f64 arithmetic, f32 result"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = np.asarray(K_from, np.float64)[:4]
    gx, gy, dx, dy = np.asarray(K_to, np.float64)[:4]
    return np.stack([(uv[:, 0] - cx) / fx * gx + dx, (uv[:, 1] - cy) / fy * gy + dy], 1).astype(np.float32)


def recamera_problem(problem, K_to, K_from=KITTI):
    """a synth.pnp_problem / ba_window / ba_window_fast dict with its pixels moved to camera K_to (everything else shared)"""
    out = dict(problem)
    out["uv"] = recamera(problem["uv"], K_from, K_to)
    return out


def swap_pose(T):
    """(S R S, S t) of poses (..., 7) = unit quaternion xyzw + translation, S the exchange of x and y.  S is a reflection, so
    S R(axis a, angle th) S = R(S a, -th): the quaternion (x, y, z, w) becomes (-y, -x, -z, w); S R S is a proper rotation."""
    T = np.asarray(T, np.float64)
    out = np.empty_like(T)
    out[..., 0] = -T[..., 1]; out[..., 1] = -T[..., 0]; out[..., 2] = -T[..., 2]; out[..., 3] = T[..., 3]
    out[..., 4] = T[..., 5]; out[..., 5] = T[..., 4]; out[..., 6] = T[..., 6]
    return out


def swap_points(xyz):
    return np.ascontiguousarray(np.asarray(xyz)[..., [1, 0, 2]])


def swap_pixels(uv):
    return np.ascontiguousarray(np.asarray(uv)[..., [1, 0]])


def swap_K(K):
    K = np.asarray(K, np.float64)
    return np.concatenate([K[[1, 0, 3, 2]], K[4:]])


def swap_model(m):
    """an EPnP model [R | t] (12,) under the exchange: (S R S, S t)"""
    m = np.asarray(m, np.float64)
    R = m[:9].reshape(3, 3)[[1, 0, 2]][:, [1, 0, 2]]
    return np.concatenate([R.reshape(9), m[9:][[1, 0, 2]]])


# columns of a pose Jacobian under the exchange: tangent [upsilon; omega], upsilon' = S upsilon, omega' = -S omega (omega is axial)
POSE_COLS = np.array([1, 0, 2, 4, 3, 5])
POSE_SIGN = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])
LM_COLS = np.array([1, 0, 2])


def swap_xy(problem, K):
    """the problem with x and y exchanged: points (Y, X, Z), pixels (v, u), K (fy, fx, cy, cx), every pose (S R S, S t).
    Returns (problem', K')."""
    out = dict(problem)
    out["xyz"] = swap_points(problem["xyz"])
    out["uv"] = swap_pixels(problem["uv"])
    for k in _POSE_KEYS:
        if k in problem:
            out[k] = swap_pose(problem[k])
    return out, swap_K(K)


def stereo_pixels(cam, seed=0, n=2000, row_errors=False):
    """the matched left / right pixels of test_gpu_geom.test_triangulate_parity (depths 2-600 m, 0.3 px noise in both coordinates, five pairs with
    zero disparity) with the disparities of `cam`, and that test's pose: (uvL, uvR, T_c_w).  row_errors: every tenth pair is additionally off
    its row by up to 6 px (0.3 px of noise never reaches a row tolerance of 2 px: without them no flag depends on whether the gate is on)."""
    from stereo_visual_slam_amd import synth
    rng = np.random.default_rng(seed)
    Z = rng.uniform(2, 600, n)
    uL = rng.uniform(0, 1241, n); v = rng.uniform(0, 376, n)
    uvL = np.stack([uL, v], 1).astype(np.float32)
    uvR = np.stack([uL - cam[0] * cam[4] / Z + rng.normal(0, 0.3, n), v + rng.normal(0, 0.3, n)], 1).astype(np.float32)
    uvR[:5] = uvL[:5]  # zero disparity -> invalid
    if row_errors:
        uvR[::10, 1] += np.random.default_rng(seed + 77).uniform(-6, 6, len(uvR[::10])).astype(np.float32)
    T = synth.perturb_pose(synth.se3_from_Rt(np.eye(3), [0.3, -0.1, 2.0]), rng, 0.2)
    return uvL, uvR, T
