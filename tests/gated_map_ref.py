"""CPU restatement of throughput mode with insert_key_frame's keyframe gate INSIDE the map-based pose passes (KeyframePipeline(pose_inputs="map",
keyframe_gate="per_pass"); vslam_gate_states_dev, vslam_build_map_pnp_inputs_gated_dev, vslam_build_windows_map_gated_dev), for the tests.

Written from the reference, not from the kernels: a Map kept in time order, the way VO / Map do it:
  motion_estimation        visual_odometry.cpp:260-277  the inputs are every feature of the last frame that the current frame matched, in match
                                                        order, each at its landmark's map position pt_3d_ (the creation point, or the first reliable
                                                        one), and the current keypoint; solvePnPRansac gives T_c_w, the inliers and num_inliers_
  tracking                 :306                         the outliers are erased from the frame: the inliers are the tracked features of the frame
  T_c_l_                   :615                         T_c_w(f) o T_c_w(f - 1)^-1
  check_motion_estimation  :316-346, insert_key_frame's gate :353   kf_gate_ref.frame_state (2 keyframe, 1 tracked, 0 rejected)
  insert_key_frame         :363-424                     at a KEYFRAME only: every feature adds an observation, a tracked feature with a reliable depth
                                                        updates an unreliable landmark (:391-401), every other keypoint with a valid depth creates one
                                                        at the frame's pose; at a non-keyframe the tracked inliers pass through and nothing is recorded
  Map::remove_keyframe     map.cpp:48-130               policy 1 (kf_gate_ref._evict); policy 0 evicts the oldest keyframe
Throughput-mode conventions (include/vslam_hip.h): frame 0 is a keyframe, a rejected frame passes through like a tracked one (status bit 2),
frame_gap 1, window b is the map right after keyframe b (empty at any other step).
Two entry points, both with a pluggable solver(i, xyz_w (n, 3) f32, uv (n, 2) f32, guess (7,)) -> (T_c_w (7,), inlier mask (n,)); num_inliers = the
mask's count:
  sequential(...)  the loop f = 1 .. F - 1 (include/vslam_hip.h, steps 1-5)
  passes(...)      pass 0 = the own-depth pose stage (its flags and track_rule on the chain of T_rel, its states from its own inlier counts and T_rel);
                   pass k walks the tracks with states^{k-1} on (G^{k-1}, links^{k-1}), solves every frame (failure rule: with no inlier
                   G^k_f = G^{k-1}_{f-1} and no links), and takes states^k from its own counts and G^k.
Windows come out in the comparison form of kf_gate_ref ({sorted observations (slot, u, v): (position, reliable)}).
"""
import numpy as np

from kf_gate_ref import IDENT, K_KITTI, _evict, _Landmark, _world, frame_state, frame_states, se3_inv, se3_mul
from pose_map_ref import chain, map_links, pass0_links


def gate(num_inliers, G_f, G_l):
    """state of frame f >= 1: the gate (:353) on num_inliers_ and T_c_l_ = G_f o G_l^-1 (:615), G_l = the last frame's T_c_w"""
    return frame_state(int(num_inliers), se3_mul(G_f, se3_inv(G_l)))


def _walk(tables, G, states=None, decide=None, solve=None, n_kf=10, policy=0, near_dist=0.2):
    """the Map in time order on the poses G (F x 7) and the frame states (F; None: computed by the gate after each solve).  Per frame pair i -> i + 1
    the map inputs (index map, xyz, uv); the links out of them are decide(i, k, j_own, lid, t, pos, G) per input (j_own: its rank among the own-depth
    matches, None without a depth), or -- `solve` -- the frame's pose is solved on them first and its state gated (sequential loop).
    Returns G (solved rows filled in), state, items, windows, kf_frame, evicted, n_kf, status."""
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, _ = tables
    F, kp_cap = kps.shape
    lr_cap = lr.shape[1]
    match_cap = f2f.shape[1] if F > 1 else 1
    G = np.array(G, np.float64, copy=True)
    state = np.full(F, 2, np.int32) if states is None else np.array(states, np.int32, copy=True)
    state[0] = 2                    # (initialization)
    L, S, windows, items, status = [], [], [], [], 0
    kf_frame = np.full((F, n_kf), -1, np.int32); evicted = np.full(F, -1, np.int32); nkf = np.zeros(F, np.int32)
    prev_feats, prev_k2 = {}, {}
    for f in range(F):
        k2 = {}
        for m in range(min(max(int(nlr[f]), 0), lr_cap)):
            q = int(lr["queryIdx"][f, m])
            if 0 <= q < kp_cap:
                k2[q] = m
        feats = {}
        if f > 0:                   # motion_estimation: the last frame's features that the current frame matched, at their landmarks' positions
            i = f - 1
            index = np.full(match_cap, -1, np.int32)
            X, U, rec, j_own = [], [], [], 0
            for k in range(min(max(int(nf2f[i]), 0), match_cap)):
                q, t = int(f2f["queryIdx"][i, k]), int(f2f["trainIdx"][i, k])
                if not (0 <= q < kp_cap and 0 <= t < kp_cap):
                    continue
                li = prev_k2.get(q, -1)
                jo = None
                if li >= 0 and valid[i, li]:
                    jo = j_own; j_own += 1
                lid = prev_feats.get(q)
                if lid is None:     # no feature (a non-keyframe's untracked keypoints are none): no input, no link
                    continue
                index[k] = len(X)
                X.append(L[lid].pt()); U.append((kps["x"][f, t], kps["y"][f, t])); rec.append((k, jo, lid, t))
            X = np.array(X, np.float32).reshape(-1, 3); U = np.array(U, np.float32).reshape(-1, 2)
            if solve is not None:
                T, mask = solve(i, X, U, G[f - 1])
                mask = np.asarray(mask, bool).reshape(len(X))
                if mask.any():
                    G[f] = T
                else:               # no model: the last pose, no links
                    G[f] = G[f - 1]; mask = np.zeros(len(X), bool)
                state[f] = gate(mask.sum(), G[f], G[f - 1])
            else:
                mask = np.array([bool(decide(i, k, jo, lid, t, X[j], G)) for j, (k, jo, lid, t) in enumerate(rec)], bool)
            items.append(dict(index=index, xyz=X, uv=U, mask=mask.astype(np.uint8), n=len(X)))
            for ok, (_, _, lid, t) in zip(mask, rec):
                if ok:              # :306 the inliers are the current frame's tracked features
                    feats[t] = lid
            if state[f] == 0:
                status |= 4
        if state[f] == 2:           # insert_key_frame (:363-424)
            for t, lid in feats.items():
                L[lid].obs.append((f, t))
            for i_ in range(kp_cap):
                m = k2.get(i_)
                if m is None or not valid[f, m]:
                    continue
                r = bool(rel[f, m]); lid = feats.get(i_)
                if lid is not None:
                    if L[lid].rel_pos is None and r:
                        L[lid].rel_pos = _world(G[f], xyz[f, m])
                    continue
                L.append(_Landmark(_world(G[f], xyz[f, m]), r, f, i_))
                feats[i_] = len(L) - 1
            S = S + [f]
            if len(S) > n_kf:
                e, fb, _ = _evict(S, G, f, policy, near_dist)
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
        else:                       # a non-keyframe: the inliers pass through, nothing is recorded, the window is empty
            windows.append({})
        kf_frame[f, :len(S)] = S
        prev_feats, prev_k2 = feats, k2
    return dict(G=G, state=state, items=items, windows=windows, kf_frame=kf_frame, evicted=evicted, n_kf=nkf, status=status)


def sequential(tables, solver, n_kf=10, policy=0, near_dist=0.2):
    """the loop f = 1 .. F - 1: frame f is solved against the map as of frame f - 1, gated, then inserted if it is a keyframe"""
    F = len(tables[0])
    G = np.tile(IDENT, (F, 1))
    return _walk(tables, G, solve=solver, n_kf=n_kf, policy=policy, near_dist=near_dist)


def states0(tables, num_inliers0):
    """states^0: the gate on the pose stage's inlier counts (item i = frame i + 1) and relative poses -- vslam_build_windows_gated_dev's states"""
    F = len(tables[0])
    return frame_states(num_inliers0, tables[9]) if F > 1 else np.array([2], np.int32)


def passes(tables, solver, K_passes, num_inliers0, G0=None, n_kf=10, policy=0, near_dist=0.2, K=K_KITTI, reproj_thr=4.0, track_rule=1):
    """K_passes refinement passes from pass 0 (G0 = the chain of T_rel unless given; links = pose_map_ref.pass0_links; states = states0).  Returns
    dict: G (= G^K), state (= states^K), per_pass (list of {items: the pass's inputs with the solver's masks, G: G^k, state: states^k, num_inliers}),
    state0, and the windows / kf_frame / evicted / n_kf / status built on (G^K, links^K, states^K)."""
    F = len(tables[0])
    G = chain(tables[9], F) if G0 is None else np.array(G0, np.float64)
    st = states0(tables, num_inliers0)
    decide = pass0_links(tables, K, reproj_thr, track_rule)
    per_pass = []
    for _ in range(K_passes):
        items = _walk(tables, G, st, decide=decide, n_kf=1)["items"]
        Gn = G.copy()
        Gn[0] = IDENT
        for i, it in enumerate(items):
            T, mask = solver(i, it["xyz"], it["uv"], G[i + 1])
            mask = np.asarray(mask, bool).reshape(it["n"])
            if mask.any():
                Gn[i + 1] = T
            else:
                Gn[i + 1] = G[i]; mask = np.zeros(it["n"], bool)
            it["mask"] = mask.astype(np.uint8)
        ninl = np.array([int(it["mask"].sum()) for it in items], np.int32)
        sn = np.array([2] + [gate(ninl[f - 1], Gn[f], Gn[f - 1]) for f in range(1, F)], np.int32)
        per_pass.append(dict(items=items, G=Gn, state=sn, num_inliers=ninl))
        decide, G, st = map_links(items), Gn, sn
    out = _walk(tables, G, st, decide=decide, n_kf=n_kf, policy=policy, near_dist=near_dist)
    out["per_pass"] = per_pass
    out["state0"] = states0(tables, num_inliers0)
    return out


def gate_solver(i, xyz, uv, guess):
    """a deterministic stand-in for the pose solver that straddles the gate's 80 inliers: a pure function of the inputs' uv and order (never of xyz).
    Inliers: a hash of each input's pixel and rank, nine in ten; no model when fewer than 3; pose: a small motion from the inliers' mean pixel and
    count -- a rotation about y of (mean u - 620) 1e-3 rad, so that T_c_l's angleY crosses 0.03 for some pairs"""
    n = len(uv)
    if n == 0:
        return IDENT.copy(), np.zeros(0, bool)
    u = uv.astype(np.float64)
    h = (np.floor(u[:, 0]).astype(np.int64) * 31 + np.floor(u[:, 1]).astype(np.int64) * 17 + np.arange(n) * 7) % 10
    mask = h < 9
    if mask.sum() < 3:
        return IDENT.copy(), np.zeros(n, bool)
    m = u[mask].mean(0)
    a = (m[0] - 620.0) * 1e-3
    T = np.array([0.0, np.sin(a / 2), 0.0, np.cos(a / 2), (m[1] - 188.0) * 1e-3, 0.01 * (i % 5), 0.5 + 1e-3 * int(mask.sum())])
    return T, mask
