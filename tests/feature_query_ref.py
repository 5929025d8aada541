"""CPU restatement of the gated map passes with the REFERENCE'S QUERY SET (KeyframePipeline(pose_inputs="map", keyframe_gate="per_pass",
f2f_queries="features"); vslam_build_map_pnp_inputs_requery_dev), for the tests.

Written from the reference like tests/gated_map_ref.py, whose Map bookkeeping, gate and conventions it reuses:
  tracking            visual_odometry.cpp:568-575  descriptors_last is built from frame_last_.features_ ONLY: after a non-keyframe the PnP inliers
                                                   that survived :306, after a keyframe those plus the landmarks insert_key_frame created
  feature_matching    :219-251                     cross-check and the max(2 d_min, 30 frame_gap) gate run on THAT subset: here the oracle's matcher on
                                                   the gathered descriptor rows (ascending keypoint index), queryIdx mapped back
  motion_estimation   :260-277                     every match of that table is an input (its query is a feature by construction)
The rest -- insert_key_frame at keyframes only, the gate, the keyframe sets, windows in kf_gate_ref's comparison form, a rejected frame passing
through, frame_gap 1 -- is gated_map_ref's.  `tables` is its tuple (kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nkps); f2f / nf2f / inl are
the pose stage's ALL-KEYPOINT table and flags (pass 0).  `match(i, sel)` returns the table of pair i -> i + 1 for the ascending query rows `sel`
of frame i as a DMATCH array (oracle_matcher below); the solver is pluggable as there.
  sequential(...)  the loop f = 1 .. F - 1: table of pair f - 1 from the features of f - 1, inputs, solve, gate, insert
  passes(...)      pass 0 = the pose stage; pass k walks with states^{k-1} on (G^{k-1}, table^{k-1}, links^{k-1}), re-matches every pair on the
                   features that walk finds (table^k), emits the inputs on table^k and solves; links^k are the masks on table^k.
Both return gated_map_ref's dict plus tables (per pair: the DMATCH array) and feats (per frame: the ascending feature list).
"""
import numpy as np

from gated_map_ref import gate, states0
from kf_gate_ref import IDENT, K_KITTI, _evict, _Landmark, _world
from pose_map_ref import chain, pass0_links


def oracle_matcher(O, desc, nkps):
    """match(i, sel): oracle.feature_matching on the gathered rows desc[i][sel] against every keypoint of frame i + 1, queryIdx mapped back"""
    def match(i, sel):
        sel = np.asarray(sel, np.int64)
        nt = int(nkps[i + 1])
        if len(sel) == 0 or nt == 0:
            return np.zeros(0, O.DMATCH_DTYPE)
        m = O.feature_matching(np.ascontiguousarray(desc[i][sel]), np.ascontiguousarray(desc[i + 1][:nt]), 1.0)
        m["queryIdx"] = sel[m["queryIdx"]]
        return m
    return match


def fixed_tables(tables):
    """match(i, sel) that ignores the selection and returns pair i of the given table: with every keypoint a feature the model is gated_map_ref's"""
    f2f, nf2f = tables[6], tables[7]
    return lambda i, sel: f2f[i, :int(nf2f[i])].copy()


def _walk(tables, G, match, states=None, link_tables=None, decide=None, solve=None, n_kf=10, policy=0, near_dist=0.2, rematch=True):
    """gated_map_ref._walk with the pair's table produced inside the loop.  Per pair i -> i + 1: the features of frame i (ascending), table =
    match(i, features), the inputs = every match of it.  Links into frame i + 1: `solve` -- the solver's mask on those inputs (sequential loop);
    else decide(i, k, j_own, lid, t, pos, G) per match k of link_tables[i], the table the previous pass solved on.  rematch False: no table, no
    inputs (the window walk after the last pass)."""
    kps, lr, nlr, xyz, valid, rel, _, _, _, _, nkps = tables
    F, kp_cap = kps.shape
    lr_cap = lr.shape[1]
    G = np.array(G, np.float64, copy=True)
    state = np.full(F, 2, np.int32) if states is None else np.array(states, np.int32, copy=True)
    state[0] = 2
    L, S, windows, items, status, new_tables, feat_lists = [], [], [], [], 0, [], []
    kf_frame = np.full((F, n_kf), -1, np.int32); evicted = np.full(F, -1, np.int32); nkf = np.zeros(F, np.int32)
    prev_feats, prev_k2 = {}, {}
    for f in range(F):
        k2 = {}
        for m in range(min(max(int(nlr[f]), 0), lr_cap)):
            q = int(lr["queryIdx"][f, m])
            if 0 <= q < kp_cap:
                k2[q] = m
        feats = {}
        if f > 0:
            i = f - 1
            X = np.zeros((0, 3), np.float32); U = np.zeros((0, 2), np.float32); tab = None
            if rematch:             # tracking :568-575 + feature_matching: the last frame's features are the query set
                tab = match(i, feat_lists[i])
                new_tables.append(tab)
                lids = [prev_feats[int(q)] for q in tab["queryIdx"]]
                X = np.array([L[lid].pt() for lid in lids], np.float32).reshape(-1, 3)
                U = np.array([(kps["x"][f, int(t)], kps["y"][f, int(t)]) for t in tab["trainIdx"]], np.float32).reshape(-1, 2)
            if solve is not None:
                T, mask = solve(i, X, U, G[f - 1])
                mask = np.asarray(mask, bool).reshape(len(X))
                if mask.any():
                    G[f] = T
                else:
                    G[f] = G[f - 1]; mask = np.zeros(len(X), bool)
                state[f] = gate(mask.sum(), G[f], G[f - 1])
                for ok, lid, t in zip(mask, lids, tab["trainIdx"]):
                    if ok:
                        feats[int(t)] = lid
            else:                   # the previous pass's links, on the table it solved on
                mask = np.zeros(len(X), np.uint8)
                old = link_tables[i]
                j_own = 0
                for k in range(len(old)):
                    q, t = int(old["queryIdx"][k]), int(old["trainIdx"][k])
                    if not (0 <= q < kp_cap and 0 <= t < kp_cap):
                        continue
                    li = prev_k2.get(q, -1)
                    jo = None
                    if li >= 0 and valid[i, li]:
                        jo = j_own; j_own += 1
                    lid = prev_feats.get(q)
                    if lid is not None and decide(i, k, jo, lid, t, L[lid].pt(), G):
                        feats[t] = lid
            if rematch:
                items.append(dict(index=np.arange(len(X), dtype=np.int32), xyz=X, uv=U, mask=np.asarray(mask, np.uint8), n=len(X)))
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
        else:
            windows.append({})
        kf_frame[f, :len(S)] = S
        feat_lists.append(np.array(sorted(feats), np.int32))
        prev_feats, prev_k2 = feats, k2
    return dict(G=G, state=state, items=items, windows=windows, kf_frame=kf_frame, evicted=evicted, n_kf=nkf, status=status, tables=new_tables,
                feats=feat_lists)


def sequential(tables, match, solver, n_kf=10, policy=0, near_dist=0.2):
    F = len(tables[0])
    return _walk(tables, np.tile(IDENT, (F, 1)), match, solve=solver, n_kf=n_kf, policy=policy, near_dist=near_dist)


def _item_links(items):
    """links^k on table^k: match k was input k (every match of a feature-query table is an input); it holds when the solver kept it"""
    return lambda i, k, jo, lid, t, pos, G: k < len(items[i]["mask"]) and items[i]["mask"][k] != 0


def passes(tables, match, solver, K_passes, num_inliers0, G0=None, n_kf=10, policy=0, near_dist=0.2, K=K_KITTI, reproj_thr=4.0, track_rule=1):
    """K_passes passes from pass 0 (the chain of T_rel, pose_map_ref.pass0_links on the all-keypoint table, gated_map_ref.states0).  Returns the
    windows etc. on (G^K, table^K, links^K, states^K), per_pass (items, G, state, num_inliers, tables, feats of every pass) and state0."""
    F = len(tables[0])
    f2f, nf2f = tables[6], tables[7]
    G = chain(tables[9], F) if G0 is None else np.array(G0, np.float64)
    st = states0(tables, num_inliers0)
    decide = pass0_links(tables, K, reproj_thr, track_rule)
    link_tables = [f2f[i, :min(max(int(nf2f[i]), 0), f2f.shape[1])] for i in range(F - 1)]
    per_pass = []
    for _ in range(K_passes):
        w = _walk(tables, G, match, st, link_tables=link_tables, decide=decide, n_kf=1)
        items = w["items"]
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
        per_pass.append(dict(items=items, G=Gn, state=sn, num_inliers=ninl, tables=w["tables"], feats=w["feats"]))
        decide, link_tables, G, st = _item_links(items), w["tables"], Gn, sn
    out = _walk(tables, G, match, st, link_tables=link_tables, decide=decide, n_kf=n_kf, policy=policy, near_dist=near_dist, rematch=False)
    out["per_pass"] = per_pass
    out["state0"] = states0(tables, num_inliers0)
    return out
