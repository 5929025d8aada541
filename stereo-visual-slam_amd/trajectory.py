"""The trajectory of a throughput-mode batch: every keyframe's pose as the BA windows left it, in the order the reference writes them.

The reference writes a keyframe's pose when Map::remove_keyframe evicts it (map.cpp:119-121, Map::write_pose :168-197) and, at the end of
the run, the keyframes the map still holds (run_vslam.cpp:84-86).  Here a frame evicted at step b leaves window b - 1, the last window that
held it, so its pose is window b - 1's BA result at its slot there; the frames of the last window take theirs from that window.  With the keyframe
gate (vslam_build_windows_gated_dev) only a keyframe step's window carries BA poses: "the last window that held it" is then the last such window
before b, and the trajectory holds keyframes only.  Pure numpy: the inputs are the keyframe sets of vslam_build_windows_kf_dev /
vslam_build_windows_gated_dev (or of the sliding window) and the BA-refined window poses.
"""
import numpy as np


def sliding_keyframes(B, n_kf):
    """the keyframe sets of the sliding window: kf_frame (B, n_kf) with -1 in unused slots, evicted (B,) = b - n_kf (-1 while negative)"""
    b = np.arange(B)[:, None]
    f = np.maximum(b - n_kf + 1, 0) + np.arange(n_kf)[None, :]
    kf_frame = np.where(f <= b, f, -1).astype(np.int32)
    evicted = np.where(np.arange(B) >= n_kf, np.arange(B) - n_kf, -1).astype(np.int32)
    return kf_frame, evicted


def assemble_trajectory(kf_frame, evicted, ba_T, window_valid=None):
    """kf_frame (B, n_kf) int: window b's frames ascending (-1 unused); evicted (B,) int: the frame evicted at step b (-1 none);
    ba_T (B, n_kf, 7): the windows' poses (T_c_w, slot k = kf_frame[b, k]); window_valid (B,) bool or None (every window): whether window b
    carries BA poses (the gate's keyframe steps).  Returns (frame_ids, T_c_w): the frames in write order -- each evicted frame at its eviction,
    from the last valid window before it, then the last valid window's frames ascending -- and (len(frame_ids), 7) their poses, row i for
    frame_ids[i]."""
    kf_frame = np.asarray(kf_frame); evicted = np.asarray(evicted); ba_T = np.asarray(ba_T, np.float64)
    B = kf_frame.shape[0]
    valid = np.ones(B, bool) if window_valid is None else np.asarray(window_valid, bool)
    ids, poses = [], []
    last = -1   # the last valid window before step b
    for b in range(1, B):
        if valid[b - 1]:
            last = b - 1
        e = int(evicted[b])
        if e < 0:
            continue
        slot = np.flatnonzero(kf_frame[last] == e) if last >= 0 else []
        if len(slot) != 1:
            raise ValueError("frame %d evicted at step %d is not in window %d" % (e, b, last))
        ids.append(e); poses.append(ba_T[last, int(slot[0])])
    if B > 0 and valid[B - 1]:
        last = B - 1
    if last >= 0:
        for k, f in enumerate(kf_frame[last]):
            if f >= 0:
                ids.append(int(f)); poses.append(ba_T[last, k])
    return np.array(ids, np.int64), (np.stack(poses) if poses else np.zeros((0, 7)))


def assemble_trajectories(kf_frame, evicted, ba_T, first, window_valid=None):
    """assemble_trajectory for a batch of independent sequences laid back to back (vslam_set_segments): first = [0, ..., B], segment s = frames
    [first[s], first[s + 1]); kf_frame / evicted hold batch frame indices, as the segmented builders write them.  Returns one (frame_ids, T_c_w)
    per segment, the ids local to the segment (frame first[s] is 0): what assemble_trajectory gives for that segment's batch alone."""
    kf_frame = np.asarray(kf_frame); evicted = np.asarray(evicted); ba_T = np.asarray(ba_T, np.float64)
    first = np.asarray(first, np.int64)
    if first.ndim != 1 or first.size < 2 or first[0] != 0 or first[-1] != kf_frame.shape[0] or (np.diff(first) <= 0).any():
        raise ValueError("first must ascend strictly from 0 to the number of windows (%d): %r" % (kf_frame.shape[0], first.tolist()))
    out = []
    for lo, hi in zip(first[:-1], first[1:]):
        kf, ev = kf_frame[lo:hi], evicted[lo:hi]
        if ((kf >= 0) & ((kf < lo) | (kf >= hi))).any() or ((ev >= 0) & ((ev < lo) | (ev >= hi))).any():
            raise ValueError("the keyframe sets of segment [%d, %d) reach outside it" % (lo, hi))
        out.append(assemble_trajectory(np.where(kf >= 0, kf - lo, -1), np.where(ev >= 0, ev - lo, -1), ba_T[lo:hi],
                                       None if window_valid is None else np.asarray(window_valid, bool)[lo:hi]))
    return out


def _rotmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def T_w_c_rows(T_c_w):
    """(N, 7) T_c_w (quaternion x, y, z, w, then translation) -> (N, 12): the row-major 3 x 4 [R | t] of T_w_c = T_c_w^-1"""
    T_c_w = np.asarray(T_c_w, np.float64).reshape(-1, 7)
    out = np.zeros((len(T_c_w), 12))
    for n, T in enumerate(T_c_w):
        R = _rotmat(T[:4] / np.linalg.norm(T[:4]))
        Rt = R.T
        out[n] = np.concatenate([Rt, (-Rt @ T[4:])[:, None]], axis=1).ravel()
    return out


def write_trajectory(path, frame_ids, T_c_w):
    """one line per frame, the format of Map::write_pose (host/map_host.cpp): the frame id, then the row-major 3 x 4 T_w_c, each number as a C++
    stream prints a double (6 significant digits)"""
    rows = T_w_c_rows(T_c_w)
    with open(path, "w") as fh:
        for f, r in zip(frame_ids, rows):
            fh.write("%d %s\n" % (int(f), " ".join("%g" % v for v in r)))


def read_trajectory(path):
    """the inverse of write_trajectory: (frame_ids (N,), T_w_c rows (N, 12))"""
    ids, rows = [], []
    with open(path) as fh:
        for line in fh:
            v = line.split()
            if v:
                ids.append(int(v[0])); rows.append([float(x) for x in v[1:13]])
    return np.array(ids, np.int64), np.array(rows, np.float64).reshape(-1, 12)
