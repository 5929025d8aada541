"""CPU restatement of the gated map passes with the REFERENCE'S FAILURE HANDLING (KeyframePipeline(rejected_frames="recover");
vslam_frame_pairs_dev, vslam_feature_matching_pairs_dev, vslam_gate_states_pairs_dev, vslam_build_map_pnp_inputs_recover_dev,
vslam_build_windows_map_recover_dev), for the tests.

Written from the reference like tests/feature_query_ref.py, whose Map bookkeeping and conventions it reuses:
  tracking                 visual_odometry.cpp:630-637  when check_motion_estimation fails move_frame() is not called: the rejected frame and its
                                                        features are dropped, frame_last_ stays the last ACCEPTED frame
  feature_matching         :239-242                     frame_gap = frame_current_.frame_id_ - frame_last_.frame_id_ widens the gate to
                                                        max(2 d_min, 30 frame_gap): here the oracle's matcher called with the pair's real gap
  check_motion_estimation  :328-329                     |log T_c_l| <= 5 frame_gap: kf_gate_ref.check_motion(..., frame_gap)
  tracking                 :673-693, run_vslam.cpp:78-81  more than ten consecutive rejections: Lost, and the node loop ends (state 3, absorbing)
`tables` is gated_map_ref's tuple; `match(l, f, sel, gap)` returns the table of the pair l -> f for the ascending query rows `sel` of frame l at
frame_gap `gap` as a DMATCH array (oracle_matcher below); the solver is pluggable as there: solver(i, xyz, uv, guess), item i = frame i + 1.
  pairs(states)    every frame's last accepted predecessor, the gap to it and the Lost frames (vslam_frame_pairs_dev's rule)
  sequential(...)  the loop of include/vslam_hip.h: last / lost_run, table of frame f from the features of `last` at gap f - last
  passes(...)      pass 0 = the pose stage on adjacent frames; pass k pairs the frames by states^{k-1}, walks (G^{k-1}, table^{k-1}, links^{k-1}) -- a
                   pair's links hold only when table^{k-1} was built on the same pairing --, re-matches, solves, gates at the pair's gap and scans Lost.
Both return feature_query_ref's dict plus pred (F), gap (F - 1) and state 3 for Lost frames; status gains bit 3 (value 8) when a frame is Lost.
"""
import numpy as np

from gated_map_ref import states0
from kf_gate_ref import IDENT, K_KITTI, _evict, _Landmark, _world, angle_y, check_motion, se3_inv, se3_mul
from pose_map_ref import chain, pass0_links

LOST_RUN = 10   # more than this many consecutive rejections: Lost (:673)


def oracle_matcher(O, desc, nkps):
    """match(l, f, sel, gap): oracle.feature_matching on the gathered rows desc[l][sel] against every keypoint of frame f at that gap, queryIdx mapped back"""
    def match(l, f, sel, gap):
        sel = np.asarray(sel, np.int64)
        nt = int(nkps[f])
        if len(sel) == 0 or nt == 0:
            return np.zeros(0, O.DMATCH_DTYPE)
        m = O.feature_matching(np.ascontiguousarray(desc[l][sel]), np.ascontiguousarray(desc[f][:nt]), float(gap))
        m["queryIdx"] = sel[m["queryIdx"]]
        return m
    return match


def adjacent(match):
    """feature_query_ref's match(i, sel) from match(l, f, sel, gap)"""
    return lambda i, sel: match(i, i + 1, sel, 1.0)


def gate(num_inliers, G_f, G_l, gap):
    """state of frame f: check_motion_estimation at the pair's gap, then insert_key_frame's 80-inlier / angleY test (2 keyframe, 1 tracked, 0 rejected)"""
    T = se3_mul(G_f, se3_inv(G_l))
    if not check_motion(int(num_inliers), T, float(gap)):
        return 0
    return 1 if (num_inliers >= 80 and angle_y(T) < 0.03) else 2


def pairs(states):
    """(pred, gap, eff): pred[f] = the last frame j < f of state 1 or 2 (frame 0 counts), -1 for frame 0 and from the first Lost frame on (11 or more
    frames of another state directly before it); gap[f - 1] = f - pred[f] (1.0 without one); eff = the states with 3 from the first Lost frame on"""
    st = np.asarray(states, np.int32)
    F = len(st)
    pred = np.full(F, -1, np.int32); gap = np.ones(max(F - 1, 0), np.float64); eff = st.copy()
    if F:
        eff[0] = 2
    last, lost = 0, False
    for f in range(1, F):
        if f - last > LOST_RUN + 1:
            lost = True
        if lost:
            eff[f] = 3
            continue
        pred[f] = last; gap[f - 1] = f - last
        if st[f] in (1, 2):
            last = f
        elif not 0 <= st[f] <= 3:
            eff[f] = 0
    return pred, gap, eff


def lost_scan(raw):
    """the states with 3 from the first Lost frame on"""
    return pairs(raw)[2]


def fallback_frames(pred):
    """the frame whose pose an item without inliers keeps: pred(f), and for a Lost frame the last accepted frame before the run"""
    return np.maximum(np.maximum.accumulate(pred), 0)


def _k2(lr, nlr, f, kp_cap):
    k2 = {}
    for m in range(min(max(int(nlr[f]), 0), lr.shape[1])):
        q = int(lr["queryIdx"][f, m])
        if 0 <= q < kp_cap:
            k2[q] = m
    return k2


class _Map:
    """insert_key_frame (:363-424), the keyframe set and the window of a keyframe step: gated_map_ref's bookkeeping"""

    def __init__(self, tables, F, n_kf, policy, near_dist):
        self.t, self.n_kf, self.policy, self.near = tables, n_kf, policy, near_dist
        self.L, self.S, self.status = [], [], 0
        self.kf_frame = np.full((F, n_kf), -1, np.int32); self.evicted = np.full(F, -1, np.int32); self.nkf = np.zeros(F, np.int32)
        self.windows = []

    def insert(self, f, feats, k2, G):
        kps, _, _, xyz, valid, rel = self.t[:6]
        L = self.L
        for t, lid in feats.items():
            L[lid].obs.append((f, t))
        for i_ in range(kps.shape[1]):
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
        self.S = self.S + [f]
        if len(self.S) > self.n_kf:
            e, fb, _ = _evict(self.S, G, f, self.policy, self.near)
            if fb:
                self.status |= 2
            self.S.remove(e); self.evicted[f] = e
        self.nkf[f] = len(self.S)
        slot = {g: k for k, g in enumerate(self.S)}
        win = {}
        for lk in L:
            o = [(slot[g], float(kps["x"][g, kp]), float(kps["y"][g, kp])) for g, kp in lk.obs if g in slot]
            if o:
                win[tuple(sorted(o))] = (lk.pt(), int(lk.rel_pos is not None))
        self.windows.append(win)

    def step_done(self, f, keyframe):
        if not keyframe:
            self.windows.append({})
        self.kf_frame[f, :len(self.S)] = self.S

    def result(self, **kw):
        return dict(windows=self.windows, kf_frame=self.kf_frame, evicted=self.evicted, n_kf=self.nkf, status=self.status, **kw)


def _inputs(M, tables, f, tab, feats_l):
    kps = tables[0]
    lids = [feats_l[int(q)] for q in tab["queryIdx"]]
    X = np.array([M.L[lid].pt() for lid in lids], np.float32).reshape(-1, 3)
    U = np.array([(kps["x"][f, int(t)], kps["y"][f, int(t)]) for t in tab["trainIdx"]], np.float32).reshape(-1, 2)
    return lids, X, U


def _empty_item():
    return dict(index=np.zeros(0, np.int32), xyz=np.zeros((0, 3), np.float32), uv=np.zeros((0, 2), np.float32), mask=np.zeros(0, np.uint8), n=0)


def sequential(tables, match, solver, n_kf=10, policy=0, near_dist=0.2):
    """the sequential loop of include/vslam_hip.h (the recover entries), steps 1-7"""
    kps, lr, nlr = tables[0], tables[1], tables[2]
    F, kp_cap = kps.shape
    G = np.tile(IDENT, (F, 1)).astype(np.float64)
    state = np.full(F, 2, np.int32); pred = np.full(F, -1, np.int32); gap = np.ones(F - 1, np.float64)
    M = _Map(tables, F, n_kf, policy, near_dist)
    O_DM = tables[6].dtype
    items, new_tables, feat_lists, feats_of = [], [], [], {}
    last, lost_run = 0, 0
    for f in range(F):
        k2 = _k2(lr, nlr, f, kp_cap)
        feats = {}
        if f > 0:
            if lost_run > LOST_RUN:                                 # 1. Lost, absorbing
                state[f] = 3; G[f] = G[last]; M.status |= 8
                new_tables.append(np.zeros(0, O_DM)); items.append(_empty_item()); feat_lists.append(np.zeros(0, np.int32))
                M.step_done(f, False)
                continue
            l = last; g = f - l; pred[f] = l; gap[f - 1] = g       # 2. the last accepted frame's features at the pair's gap
            tab = match(l, f, feat_lists[l], g)
            new_tables.append(tab)
            lids, X, U = _inputs(M, tables, f, tab, feats_of[l])    # 3.
            T, mask = solver(f - 1, X, U, G[l])                     # 4.
            mask = np.asarray(mask, bool).reshape(len(X))
            if mask.any():
                G[f] = T
            else:
                G[f] = G[l]; mask = np.zeros(len(X), bool)
            items.append(dict(index=np.arange(len(X), dtype=np.int32), xyz=X, uv=U, mask=mask.astype(np.uint8), n=len(X)))
            state[f] = gate(mask.sum(), G[f], G[l], g)              # 5.
            if state[f] == 0:                                       # 6. dropped
                lost_run += 1; M.status |= 4
            else:                                                   # 7.
                lost_run = 0; last = f
                for ok, lid, t in zip(mask, lids, tab["trainIdx"]):
                    if ok:
                        feats[int(t)] = lid
        if state[f] == 2:
            M.insert(f, feats, k2, G)
        M.step_done(f, state[f] == 2)
        feats_of[f] = feats
        feat_lists.append(np.array(sorted(feats), np.int32))
    return M.result(G=G, state=state, items=items, tables=new_tables, feats=feat_lists, pred=pred, gap=gap)


def _walk(tables, G, match, states, pred_prev, link_tables, decide, n_kf=10, policy=0, near_dist=0.2, rematch=True):
    """one pass's walk: the pairing of `states`; the links of item f - 1 (decide(...) per match of link_tables[f - 1], the table the previous pass solved
    on, built on pred_prev) hold only for an accepted frame whose pairing did not change; the re-match of every frame with a predecessor"""
    kps, lr, nlr, _, valid = tables[:5]
    F, kp_cap = kps.shape
    pred, gap, eff = pairs(states)
    M = _Map(tables, F, n_kf, policy, near_dist)
    O_DM = tables[6].dtype
    items, new_tables, feat_lists, feats_of, k2_of = [], [], [], {}, {}
    for f in range(F):
        k2 = k2_of[f] = _k2(lr, nlr, f, kp_cap)
        feats = {}
        accepted = f == 0 or eff[f] in (1, 2)
        if f > 0:
            l = int(pred[f])
            if rematch:
                if l >= 0:
                    tab = match(l, f, feat_lists[l], gap[f - 1])
                    _, X, U = _inputs(M, tables, f, tab, feats_of[l])
                    items.append(dict(index=np.arange(len(X), dtype=np.int32), xyz=X, uv=U, mask=np.zeros(len(X), np.uint8), n=len(X)))
                else:
                    tab = np.zeros(0, O_DM); items.append(_empty_item())
                new_tables.append(tab)
            if accepted and l >= 0 and int(pred_prev[f]) == l:
                old = link_tables[f - 1]
                j_own = 0
                for k in range(len(old)):
                    q, t = int(old["queryIdx"][k]), int(old["trainIdx"][k])
                    if not (0 <= q < kp_cap and 0 <= t < kp_cap):
                        continue
                    li = k2_of[l].get(q, -1)
                    jo = None
                    if li >= 0 and valid[l, li]:
                        jo = j_own; j_own += 1
                    lid = feats_of[l].get(q)
                    if lid is not None and decide(f - 1, k, jo, lid, t, M.L[lid].pt(), G):
                        feats[t] = lid
            if eff[f] == 0:
                M.status |= 4
            if eff[f] == 3:
                M.status |= 8
        if eff[f] == 2:
            M.insert(f, feats, k2, G)
        M.step_done(f, eff[f] == 2)
        feats_of[f] = feats if accepted else {}
        feat_lists.append(np.array(sorted(feats_of[f]), np.int32))
    return M.result(G=np.array(G, np.float64), state=eff, items=items, tables=new_tables, feats=feat_lists, pred=pred, gap=gap)


def _item_links(items):
    return lambda i, k, jo, lid, t, pos, G: k < len(items[i]["mask"]) and items[i]["mask"][k] != 0


def passes(tables, match, solver, K_passes, num_inliers0, G0=None, n_kf=10, policy=0, near_dist=0.2, K=K_KITTI, reproj_thr=4.0, track_rule=1, state0=None):
    """K_passes passes from pass 0 (the chain of T_rel, pose_map_ref.pass0_links on the all-keypoint table of adjacent frames, gated_map_ref.states0
    unless state0 is given).  Returns the windows etc. on (G^K, table^K, links^K, states^K), per_pass (items, G, state, num_inliers, tables, feats, pred,
    gap of every pass) and state0."""
    F = len(tables[0])
    f2f, nf2f = tables[6], tables[7]
    G = chain(tables[9], F) if G0 is None else np.array(G0, np.float64)
    st0 = states0(tables, num_inliers0) if state0 is None else np.array(state0, np.int32)
    st = st0
    decide = pass0_links(tables, K, reproj_thr, track_rule)
    link_tables = [f2f[i, :min(max(int(nf2f[i]), 0), f2f.shape[1])] for i in range(F - 1)]
    pred_prev = np.arange(F, dtype=np.int32) - 1
    per_pass = []
    for _ in range(K_passes):
        w = _walk(tables, G, match, st, pred_prev, link_tables, decide, n_kf=1)
        items, pred, gap = w["items"], w["pred"], w["gap"]
        fb = fallback_frames(pred)
        Gn = G.copy()
        Gn[0] = IDENT
        for i, it in enumerate(items):
            T, mask = solver(i, it["xyz"], it["uv"], G[i + 1])
            mask = np.asarray(mask, bool).reshape(it["n"])
            if mask.any():
                Gn[i + 1] = T
            else:
                Gn[i + 1] = G[fb[i + 1]]; mask = np.zeros(it["n"], bool)
            it["mask"] = mask.astype(np.uint8)
        ninl = np.array([int(it["mask"].sum()) for it in items], np.int32)
        raw = np.array([2] + [gate(ninl[f - 1], Gn[f], Gn[pred[f]], f - pred[f]) if pred[f] >= 0 else 0 for f in range(1, F)], np.int32)
        sn = lost_scan(raw)
        per_pass.append(dict(items=items, G=Gn, state=sn, num_inliers=ninl, tables=w["tables"], feats=w["feats"], pred=pred, gap=gap))
        decide, link_tables, G, st, pred_prev = _item_links(items), w["tables"], Gn, sn, pred
    out = _walk(tables, G, match, st, pred_prev, link_tables, decide, n_kf=n_kf, policy=policy, near_dist=near_dist, rematch=False)
    out["per_pass"] = per_pass
    out["state0"] = st0
    return out
