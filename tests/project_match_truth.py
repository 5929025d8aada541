"""Ground truth for match by projection on rendered frames (tests/place_inputs.py): a keypoint's world point from the render depth and the render pose,
and the rule by which a match counts as correct -- the two keypoints' world points agree within max(0.05 m, 2 % of the depth).  Shared by the CPU
precision test of the yardstick and the device test of the pipeline."""
import numpy as np

# the smallest precision test_project_match_precision.py measures over its five pairs (71 of 72), rounded down: what the device test of the pipeline is held
# against (it may fall short of it by 0.05: estimated poses and stereo depth replace the render geometry).  The CPU test asserts it is still reached.
CPU_PRECISION = 0.986


def world_points(xy, depth, T_c_w, K4, R_from_quat):
    """(world points (n, 3), camera depth (n,)) of pixels xy (n, 2): the render depth at the nearest pixel, back-projected with the render pose;
    NaN where the renderer hit nothing"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    h, w = depth.shape
    c = np.clip(np.rint(xy[:, 0]).astype(int), 0, w - 1); r = np.clip(np.rint(xy[:, 1]).astype(int), 0, h - 1)
    z = np.where(np.isfinite(depth[r, c]), depth[r, c], np.nan).astype(np.float64)
    P = np.stack([(xy[:, 0] - K4[2]) / K4[0] * z, (xy[:, 1] - K4[3]) / K4[1] * z, z], 1)
    R = R_from_quat(np.asarray(T_c_w[:4], np.float64))
    return (P - np.asarray(T_c_w[4:], np.float64)) @ R, z


def correct(Wa, Wb, z):
    """per pair of world points: do they agree within max(0.05 m, 2 % of depth)?  (False where either is NaN)"""
    d = np.linalg.norm(np.asarray(Wa) - np.asarray(Wb), axis=-1)
    with np.errstate(invalid="ignore"):
        return d <= np.maximum(0.05, 0.02 * np.asarray(z))
