"""Plain numpy loops for the device glue between the matcher and the pose stage (include/vslam_hip.h: vslam_gather_matched_uv_dev,
vslam_build_pnp_inputs_dev), one item at a time, written from the header's sequential rule and not from the kernels.  Checked on two hand-worked
tables in tests/test_glue_ref.py; the yardstick of tests/test_gpu_glue.py."""
import numpy as np


def gather_uv(kpsQ, kpsT, matches, n, match_capacity):
    """kpsQ, kpsT (kp_capacity,) keypoint records, matches (match_capacity,) DMatch records, n the item's count.  Returns (rows, uvQ, uvT): the
    rows written, min(n, match_capacity) or 0 for a negative count, and their pixels (rows, 2) f32.  An index outside [0, kp_capacity) is clamped
    to that range: what the library does, pinned here."""
    kp_capacity = len(kpsQ)
    rows = max(min(int(n), int(match_capacity)), 0)
    uvQ = np.zeros((rows, 2), np.float32); uvT = np.zeros((rows, 2), np.float32)
    for i in range(rows):
        q = min(max(int(matches["queryIdx"][i]), 0), kp_capacity - 1)
        t = min(max(int(matches["trainIdx"][i]), 0), kp_capacity - 1)
        uvQ[i] = (kpsQ["x"][q], kpsQ["y"][q])
        uvT[i] = (kpsT["x"][t], kpsT["y"][t])
    return rows, uvQ, uvT


def build_pnp_inputs(f2f, nm, match_capacity, lr, nlr, lr_capacity, xyz_lr, valid_lr, kps_cur, out_capacity):
    """One item: f2f (match_capacity,) and lr (lr_capacity,) DMatch records with their counts, xyz_lr (lr_capacity, 3) f32, valid_lr (lr_capacity,),
    kps_cur (kp_capacity,) keypoint records.  Returns (kp2lr (kp_capacity,) int32, nout, xyz (nout, 3) f32, uv (nout, 2) f32)."""
    kp_capacity = len(kps_cur)
    kp2lr = np.full(kp_capacity, -1, np.int32)
    for i in range(min(int(nlr), int(lr_capacity))):
        q = int(lr["queryIdx"][i])
        if 0 <= q < kp_capacity:
            kp2lr[q] = i            # in order: the last match with this queryIdx wins
    xyz, uv = [], []
    survivors = 0
    for i in range(min(int(nm), int(match_capacity))):
        q, t = int(f2f["queryIdx"][i]), int(f2f["trainIdx"][i])
        if not (0 <= q < kp_capacity and 0 <= t < kp_capacity):
            continue
        li = int(kp2lr[q])
        if li < 0 or valid_lr[li] == 0:
            continue
        if survivors < out_capacity:
            xyz.append(xyz_lr[li].copy()); uv.append((kps_cur["x"][t], kps_cur["y"][t]))
        survivors += 1
    nout = min(survivors, int(out_capacity))
    return kp2lr, nout, np.array(xyz, np.float32).reshape(-1, 3), np.array(uv, np.float32).reshape(-1, 2)
