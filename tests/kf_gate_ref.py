"""CPU restatement of throughput mode with insert_key_frame's keyframe gate (vslam_build_windows_gated_dev), for the tests.

Written from the reference, not from the kernels: one pass over the frames in time order that keeps a Map -- landmark records with observation
lists, the current frame's features, a keyframe set -- the way VO / Map do it:
  check_motion_estimation  visual_odometry.cpp:316-346   >= 10 inliers and |log T_c_l| <= 5 (frame_gap 1)
  insert_key_frame         :353                          a keyframe unless (num_inliers >= 80 and angleY(T_c_l) < 0.03) or the check failed
  tracking                 :568-599                      the last frame's features are the query set; a match gives the current keypoint the
                                                         landmark of the matched feature (pose-stage inlier flag for a feature with a depth of its
                                                         own, else the 4 px reprojection of the landmark's map position: track_rule 1)
  insert_key_frame         :363-424                      at a keyframe only: every feature adds an observation, a tracked feature with a reliable
                                                         depth updates an unreliable landmark, every other keypoint with a valid depth creates one
  Map::remove_keyframe     map.cpp:48-130                policy 1: the nearest member if closer than near_dist, else the farthest (ties: lowest frame)
Throughput-mode conventions (include/vslam_hip.h): frame 0 is a keyframe, a rejected frame passes through like a tracked one, poses are the
pose stage's relative poses chained from frame 0, window b is the map right after keyframe b (empty at any other step), policy 0 evicts the
oldest keyframe.  Windows come out in the order-free comparison form of tests/test_gpu_windows_kf.py: {sorted observations (slot, u, v):
(position, reliable)}.
"""
import math

import numpy as np

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157])


# ------------------------------------------------------------------ SE3 (quaternion x, y, z, w, then translation; Sophus conventions)
def rotmat(T):
    x, y, z, w = np.asarray(T[:4], np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def se3_log(T):
    """Sophus::SE3d::log: [upsilon; omega]"""
    q = np.asarray(T[:4], np.float64); t = np.asarray(T[4:7], np.float64)
    v, w = q[:3], q[3]
    n2 = float(v @ v); n = math.sqrt(n2)
    if n < 1e-10:
        two_atan = 2.0 / w - 2.0 / 3.0 * n2 / (w * w * w)
    elif abs(w) < 1e-10:
        two_atan = (math.pi if w > 0 else -math.pi) / n
    else:
        two_atan = 2.0 * math.atan(n / w) / n
    om = two_atan * v
    theta = two_atan * n
    O = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if abs(theta) < 1e-10:
        c = 1.0 / 12.0
    else:
        c = (1.0 - theta * math.cos(0.5 * theta) / (2.0 * math.sin(0.5 * theta))) / (theta * theta)
    Vi = np.eye(3) - 0.5 * O + c * (O @ O)
    return np.concatenate([Vi @ t, om])


def angle_y(T):
    """Sophus::SO3d::angleY, signed"""
    R = rotmat(T)
    return math.atan2(-R[2, 0], math.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2))


def se3_mul(A, B):
    """A o B: the Hamilton product of the quaternions (normalised), A's rotation applied to B's translation plus A's"""
    ax, ay, az, aw = A[:4]; bx, by, bz, bw = B[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])
    return np.concatenate([q / np.linalg.norm(q), rotmat(A) @ np.asarray(B[4:7], np.float64) + A[4:7]])


def se3_inv(T):
    R = rotmat(T)
    return np.concatenate([[-T[0], -T[1], -T[2], T[3]], -R.T @ T[4:7]])


# ------------------------------------------------------------------ the gate
def check_motion(num_inliers, T_c_l, frame_gap=1.0):
    """VO::check_motion_estimation (:316-346)"""
    if num_inliers < 10:
        return False
    return not (np.linalg.norm(se3_log(T_c_l)) > 5.0 * frame_gap)


def frame_state(num_inliers, T_c_l):
    """2 keyframe, 1 tracked (not a keyframe), 0 rejected -- for a frame f >= 1 (frame 0 is 2)"""
    check = check_motion(num_inliers, T_c_l)
    if not check:
        return 0
    return 1 if (num_inliers >= 80 and angle_y(T_c_l) < 0.03) else 2


def frame_states(num_inliers, T_rel):
    F = len(T_rel) + 1
    return np.array([2] + [frame_state(int(num_inliers[f - 1]), T_rel[f - 1]) for f in range(1, F)], np.int32)


# ------------------------------------------------------------------ the Map simulation
class _Landmark:
    __slots__ = ("pos0", "rel_pos", "obs")

    def __init__(self, pos, reliable, f, kp):
        self.pos0 = pos
        self.rel_pos = pos if reliable else None   # pt_3d_ once reliable_depth_ is true
        self.obs = [(f, kp)]

    def pt(self):
        return self.rel_pos if self.rel_pos is not None else self.pos0


def _world(G, p_c):
    """the camera point p_c of a frame with T_c_w = G in the world, as the map stores it (float)"""
    R = rotmat(G)
    return (R.T @ (np.asarray(p_c, np.float64) - G[4:7])).astype(np.float32)


def _reprojects(pos, G, kp, K, thr):
    pc = rotmat(G) @ np.asarray(pos, np.float64) + G[4:7]
    with np.errstate(all="ignore"):
        du = float(kp["x"]) - (K[0] * pc[0] / pc[2] + K[2]); dv = float(kp["y"]) - (K[1] * pc[1] / pc[2] + K[3])
        c = du * du + dv * dv
    return bool(np.isfinite(c) and c <= thr * thr)


def _evict(S, G, b, policy, near_dist):
    """the member of S (ascending, S[-1] = b) that goes; (frame, fallback used, decision margin)"""
    if policy == 0:
        return S[0], False, np.inf
    Gi = se3_inv(G[b])
    d = [float(np.linalg.norm(se3_log(se3_mul(G[k], Gi)))) for k in S[:-1]]
    far, far_d, near, near_d = None, 0.0, None, 1e6
    for k, dk in zip(S[:-1], d):
        if dk > far_d:
            far, far_d = k, dk
        if dk < near_d:
            near, near_d = k, dk
    margin = np.inf
    if len(d) > 1:
        srt = np.sort(d)
        margin = min(srt[1] - srt[0], srt[-1] - srt[-2])
    if near is not None:
        margin = min(margin, abs(near_d - near_dist))
    if near is not None and near_d < near_dist:
        return near, False, margin
    if far is not None:
        return far, False, margin
    return S[0], True, margin


def simulate(tables, num_inliers, n_kf, policy, near_dist=0.2, K=K_KITTI, reproj_thr=4.0, track_rule=1):
    """tables = (kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk) as in tests/test_gpu_windows._random_tracks; num_inliers (F - 1,): item i
    is the pose stage's count of frame i + 1.  Returns a dict: state (F,), kf_frame (F, n_kf), evicted (F,), n_kf (F,) (0 at a non-keyframe step),
    status (bit 1: a fallback eviction, bit 2: a rejected frame; bit 0, capacity, is the caller's), G (F, 7) chained poses, windows (F dicts in the
    comparison form), margin (the smallest distance of a culling decision from flipping)"""
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, _ = tables
    F, kp_cap = kps.shape
    lr_cap = lr.shape[1]
    match_cap = f2f.shape[1] if F > 1 else 1
    pnp_cap = inl.shape[1] if F > 1 else 1
    state = frame_states(num_inliers, T_rel) if F > 1 else np.array([2], np.int32)
    G = [IDENT.copy()]
    for f in range(1, F):
        G.append(se3_mul(T_rel[f - 1], G[-1]))
    G = np.stack(G)
    L = []                          # the map's landmarks
    S = []                          # the map's keyframes (ascending frames)
    kf_frame = np.full((F, n_kf), -1, np.int32); evicted = np.full(F, -1, np.int32); nkf = np.zeros(F, np.int32)
    windows, status, margin = [], 0, np.inf
    prev_feats, prev_k2 = {}, {}
    for f in range(F):
        k2 = {}
        for m in range(min(max(int(nlr[f]), 0), lr_cap)):
            q = int(lr["queryIdx"][f, m])
            if 0 <= q < kp_cap:
                k2[q] = m
        feats = {}                  # keypoint -> landmark: the features of frame f
        if f > 0:                   # tracking: the last frame's features are the query set
            j = 0
            for k in range(min(max(int(nf2f[f - 1]), 0), match_cap)):
                q, t = int(f2f["queryIdx"][f - 1, k]), int(f2f["trainIdx"][f - 1, k])
                if not (0 <= q < kp_cap and 0 <= t < kp_cap):
                    continue
                li = prev_k2.get(q, -1); lid = prev_feats.get(q)
                if li >= 0 and valid[f - 1, li]:    # an input of the pose stage: its inlier flag decides (outliers erased, :306)
                    jj = j; j += 1
                    if jj >= pnp_cap or not inl[f - 1, jj] or lid is None:
                        continue
                else:                               # a feature without a depth of its own: PnPRansac's 4 px on the landmark's map position
                    if not track_rule or lid is None or not _reprojects(L[lid].pt(), G[f], kps[f, t], K, reproj_thr):
                        continue
                feats[t] = lid
        if f > 0 and state[f] == 0:
            status |= 4
        if state[f] == 2:           # insert_key_frame
            for t, lid in feats.items():
                L[lid].obs.append((f, t))
            for i in range(kp_cap):
                m = k2.get(i)
                if m is None or not valid[f, m]:
                    continue
                r = bool(rel[f, m]); lid = feats.get(i)
                if lid is not None:
                    if L[lid].rel_pos is None and r:
                        L[lid].rel_pos = _world(G[f], xyz[f, m])
                    continue
                L.append(_Landmark(_world(G[f], xyz[f, m]), r, f, i))
                feats[i] = len(L) - 1
            S = S + [f]
            if len(S) > n_kf:
                e, fb, mg = _evict(S, G, f, policy, near_dist)
                margin = min(margin, mg)
                if fb:
                    status |= 2
                S.remove(e); evicted[f] = e
            nkf[f] = len(S)
            slot = {g: k for k, g in enumerate(S)}
            win = {}
            for lk in L:
                o = [(slot[g], float(kps["x"][g, kp]), float(kps["y"][g, kp])) for g, kp in lk.obs if g in slot]
                if o:
                    win[tuple(sorted(o))] = (lk.pt(), int(lk.rel_pos is not None))
            windows.append(win)
        else:
            windows.append({})
        kf_frame[f, :len(S)] = S
        prev_feats, prev_k2 = feats, k2
    return dict(state=state, kf_frame=kf_frame, evicted=evicted, n_kf=nkf, status=status, G=G, windows=windows, margin=margin)


def oracle_windows(full, kf_frame):
    """oracle/windows.c's windows (full history: n_kf = F, kf_idx = frame) restricted to the sets kf_frame, in the comparison form"""
    out = []
    for b in range(len(kf_frame)):
        S = [int(f) for f in kf_frame[b] if f >= 0]
        slot = {f: k for k, f in enumerate(S)}
        l0, e0, e1 = full["lm_off"][b], full["edge_off"][b], full["edge_off"][b + 1]
        kf, lm, uv = full["kf_idx"][e0:e1], full["lm_idx"][e0:e1], full["uv"][e0:e1]
        keep = np.isin(kf, S)
        win = {}
        for l in np.unique(lm[keep]):
            sel = keep & (lm == l)
            key = tuple(sorted(zip([slot[int(f)] for f in kf[sel]], uv[sel, 0].tolist(), uv[sel, 1].tolist())))
            win[key] = (full["xyz"][l0 + l], int(full["reliable"][l0 + l]))
        out.append(win)
    return out


def same_windows(a, b, rtol=3e-6, atol=2e-5):
    """two lists of comparison-form windows agree: the same landmarks (observations), reliable flags, positions within the tolerance"""
    if len(a) != len(b):
        return False
    for wa, wb in zip(a, b):
        if wa.keys() != wb.keys():
            return False
        for k, (p, r) in wa.items():
            if wb[k][1] != r or not np.allclose(wb[k][0], p, rtol=rtol, atol=atol):
                return False
    return True
