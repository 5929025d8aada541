"""Host side of the full bundle adjustment stage: what a pipeline step leaves in, refined trajectories and a moved map out (include/vslam_hip.h
"full bundle adjustment").  FullBA only lays the arrays out -- numpy, once per step; the optimisation is VO.full_ba, one persistent workgroup per
segment on the device."""
import numpy as np

from .posegraph import se3_inverse, se3_mul, _rot


def se3_act(T, X):
    """T o X for poses (n, 7) and points (n, 3)"""
    return np.einsum("...ij,...j->...i", _rot(T), X) + T[..., 4:]


class FullBA:
    """One problem per segment of a step.

    Keyframes: the frames of the segment's trajectory, numbered along it; keyframe 0 is held.
    Observations: the union of the BA windows' observations, de-duplicated by (frame, landmark id); an observation of a frame that is no keyframe of
    its landmark's segment is left out and counted.
    Landmarks: a landmark's identity is the keypoint that created it (vslam_set_window_ids: frame x kp_capacity + keypoint); its initial position is
    the one the last window that holds it left.  The creating observation gets the disparity fx b / Z of the creating keypoint's own stereo point
    when that point is valid; every other observation is left-image-only.  A landmark left with a single mono observation is not part of the
    problem.
    Edges: the accepted rows of a LOOP_EDGE_DTYPE array whose two frames are keyframes of one segment, i = frame_q, j = frame_c, Z = T_q_c, the
    diagonal information w_loop = (translation, rotation); as for PoseGraph no measured default exists, 1.0 says a metre and a radian weigh as much
    as a pixel squared.
    Initial poses: the trajectory's, or `poses` (what close_loops returned); with `poses` every landmark is first carried rigidly by its creating
    keyframe's correction, X <- T_new^-1 T_old X (the creating frame if it is a keyframe, else the first keyframe that observes it).  Landmarks that
    are not part of the problem are carried the same way by the final correction, so the map moves as a whole.

    .report counts what was left out.  Limits: one workgroup per problem, block-Jacobi only, one world per step (frames of other steps are out of
    reach), and the result is not fed back into tracking."""

    def __init__(self, K4, bf, kp_capacity, w_loop=(1.0, 1.0), huber_delta=0.0):
        self.K4 = tuple(float(v) for v in K4); self.bf = float(bf); self.cap = int(kp_capacity)
        self.w_loop = np.repeat(np.asarray(w_loop, np.float64), 3)
        assert self.w_loop.shape == (6,)
        self.huber_delta = float(huber_delta)
        self.segs = []
        self.report = dict(observations_seen=0, observations=0, observations_duplicate=0, observations_other_segment=0, observations_dropped=0,
                           landmarks_seen=0, landmarks=0, landmarks_dropped=0, landmarks_without_stereo=0, edges_added=0, edges_not_accepted=0,
                           edges_unknown_seq=0, edges_unknown_frame=0)

    def add_segment(self, first_frame, frame_ids, T_old, obs_frame, obs_lm_id, obs_uv, lm_id, lm_xyz, kp_xyz, kp_valid, T_new=None, merge=None):
        """first_frame: the batch frame index of the segment's frame 0; frame_ids (segment-local, as trajectories() returns them) with their poses
        T_old; the windows' observations as (batch frame, landmark id, uv) and their landmarks as (id, world position), duplicates included, in window
        order; kp_xyz (B, cap, 3) / kp_valid (B, cap): the step's camera-frame stereo points per left keypoint; T_new: the initial poses in place of
        T_old.  merge = (ids, canonical), what reobserve() found: landmarks fused into classes.  The creating observation's disparity is computed
        from the ORIGINAL id, then the ids are remapped to the canonical one, the observations de-duplicated again by (frame, canonical id) -- a stereo
        row wins over a mono one -- and the class takes the canonical landmark's position: a merged class keeps every member's stereo row.  None
        leaves every array as it was before the argument existed."""
        rep = self.report
        canon = None
        if merge is not None:
            m_ids, m_can = (np.asarray(a, np.int64).reshape(-1) for a in merge)
            assert len(m_ids) == len(m_can)
            mo = np.argsort(m_ids, kind="stable"); m_ids, m_can = m_ids[mo], m_can[mo]

            def canon(a):
                if not len(m_ids) or not len(a):
                    return a
                k = np.minimum(np.searchsorted(m_ids, a), len(m_ids) - 1)
                return np.where(m_ids[k] == a, m_can[k], a)
        ids = np.asarray(frame_ids, np.int64); order = np.argsort(ids, kind="stable")
        ids = ids[order]; T_old = np.asarray(T_old, np.float64).reshape(-1, 7)[order]
        assert len(np.unique(ids)) == len(ids)
        T0 = T_old if T_new is None else np.asarray(T_new, np.float64).reshape(-1, 7)[order]
        N = len(ids)
        obs_frame = np.asarray(obs_frame, np.int64); obs_lm_id = np.asarray(obs_lm_id, np.int64); obs_uv = np.asarray(obs_uv, np.float32).reshape(-1, 2)
        lm_id = np.asarray(lm_id, np.int64); lm_xyz = np.asarray(lm_xyz, np.float64).reshape(-1, 3)
        if canon is not None:   # the canonical landmark stands for its class
            is_canon = canon(lm_id) == lm_id
            rep["landmarks_merged"] = rep.get("landmarks_merged", 0) + len(np.unique(lm_id[~is_canon]))
            lm_id, lm_xyz = lm_id[is_canon], lm_xyz[is_canon]
        rep["observations_seen"] += len(obs_frame)
        # landmarks: one per id, at the position the last window left
        uid, last = np.unique(lm_id[::-1], return_index=True)
        X_all = lm_xyz[::-1][last] if len(uid) else np.zeros((0, 3))
        rep["landmarks_seen"] += len(uid)
        # observations: first of every (frame, id); the frame must be a keyframe of this segment
        key = obs_frame * (np.int64(1) << 40) + obs_lm_id
        _, firsts = np.unique(key, return_index=True)
        firsts.sort()
        rep["observations_duplicate"] += len(key) - len(firsts)
        of, ol, ouv = obs_frame[firsts] - int(first_frame), obs_lm_id[firsts], obs_uv[firsts]
        node = np.searchsorted(ids, of); node = np.minimum(node, max(N - 1, 0))
        known = (ids[node] == of) if N else np.zeros(len(of), bool)
        rep["observations_other_segment"] += int((~known).sum())
        of, ol, ouv, node = of[known], ol[known], ouv[known], node[known]
        # the creating observation's disparity
        cf, ck = ol // self.cap, ol % self.cap
        creating = (cf - int(first_frame)) == of
        disp = np.full(len(ol), -1.0, np.float32)
        if len(ol):
            z = kp_xyz[np.clip(cf, 0, len(kp_xyz) - 1), ck, 2].astype(np.float64)
            ok = creating & (cf >= 0) & (cf < len(kp_xyz)) & (kp_valid[np.clip(cf, 0, len(kp_xyz) - 1), ck] != 0) & (z > 0)
            disp[ok] = (self.bf / z[ok]).astype(np.float32)
        if canon is not None:   # the ids to canonical, then one observation per (frame, class): the first stereo one, else the first
            ol = canon(ol)
            o2 = np.lexsort((np.arange(len(ol)), disp < 0, ol, of))
            new = np.ones(len(o2), bool); new[1:] = (of[o2][1:] != of[o2][:-1]) | (ol[o2][1:] != ol[o2][:-1])
            pick = np.sort(o2[new])
            rep["observations_merged_duplicate"] = rep.get("observations_merged_duplicate", 0) + len(ol) - len(pick)
            of, ol, ouv, node, disp = of[pick], ol[pick], ouv[pick], node[pick], disp[pick]
        # a landmark left with a single mono observation is not part of the problem
        lidx = np.searchsorted(uid, ol)
        n_obs = np.bincount(lidx, minlength=len(uid)); n_st = np.bincount(lidx[disp >= 0], minlength=len(uid))
        part = (n_obs >= 2) | (n_st >= 1)
        keep = part[lidx]
        rep["observations_dropped"] += int((~keep).sum()); rep["observations"] += int(keep.sum())
        rep["landmarks"] += int(part.sum()); rep["landmarks_dropped"] += int((~part).sum()); rep["landmarks_without_stereo"] += int((part & (n_st == 0)).sum())
        node, ouv, disp, lidx = node[keep], ouv[keep], disp[keep], lidx[keep]
        local = np.cumsum(part) - 1
        o = np.lexsort((node, local[lidx]))   # sorted by landmark, then by keyframe
        # the keyframe that carries a landmark: its creating frame if that is a keyframe, else the first keyframe that observes it, else the nearest
        cfl = uid // self.cap - int(first_frame)
        carrier = np.minimum(np.searchsorted(ids, cfl), max(N - 1, 0)) if N else np.zeros(len(uid), np.int64)
        if N:
            miss = ids[carrier] != cfl
            first_obs = np.full(len(uid), -1, np.int64)
            if len(lidx):
                oo = np.lexsort((node, lidx))
                l_sorted = lidx[oo]
                starts = np.concatenate([[True], l_sorted[1:] != l_sorted[:-1]])
                first_obs[l_sorted[starts]] = node[oo][starts]
            carrier = np.where(miss & (first_obs >= 0), first_obs, carrier)
        self.segs.append(dict(first_frame=int(first_frame), order=order, ids=ids, T_old=T_old, T0=T0, lm_id=uid, X_old=X_all, part=part, carrier=carrier,
                              kf=node[o].astype(np.int32), lm=local[lidx][o].astype(np.int32), uv=ouv[o], disp=disp[o], loops=[]))

    def add_loop_edges(self, rows, frame_offset=0):
        """the ACCEPTED rows whose two frames (batch-wide + frame_offset) are keyframes of one segment become edges; every row is counted in .report"""
        rep = self.report
        firsts = np.array([s["first_frame"] for s in self.segs], np.int64)
        ends = np.array([s["first_frame"] + (s["ids"][-1] + 1 if len(s["ids"]) else 0) for s in self.segs], np.int64)
        for row in rows:
            if not row["accepted"]:
                rep["edges_not_accepted"] += 1
                continue
            fq, fc = int(row["frame_q"]) - int(frame_offset), int(row["frame_c"]) - int(frame_offset)
            s = int(np.searchsorted(firsts, fq, side="right")) - 1
            if s < 0 or fq >= ends[s] or not (firsts[s] <= fc < ends[s]):
                rep["edges_unknown_seq"] += 1
                continue
            ids = self.segs[s]["ids"]
            q, c = np.searchsorted(ids, fq - firsts[s]), np.searchsorted(ids, fc - firsts[s])
            if q >= len(ids) or c >= len(ids) or ids[q] != fq - firsts[s] or ids[c] != fc - firsts[s] or q == c:
                rep["edges_unknown_frame"] += 1
                continue
            self.segs[s]["loops"].append((int(q), int(c), np.array(row["T_q_c"], np.float64)))
            rep["edges_added"] += 1

    def problems(self):
        """one dict per segment in the form tests/full_ba_ref.py takes (T, X, kf, lm, uv, disp, ei, ej, Z, w, fixed, obs_active, edge_active, K4, bf,
        huber): the problem as the device gets it"""
        out = []
        for s in self.segs:
            X = s["X_old"]
            if len(X):   # carried by the creating keyframe's correction (the identity when T0 is T_old)
                c = s["carrier"]
                X = se3_act(se3_mul(se3_inverse(s["T0"][c]), s["T_old"][c]), X) if len(s["ids"]) else X
            L = s["loops"]
            out.append(dict(T=s["T0"].copy(), X=X[s["part"]], kf=s["kf"], lm=s["lm"], uv=s["uv"], disp=s["disp"], fixed=None, obs_active=None, edge_active=None,
                            ei=np.array([l[0] for l in L], np.int32), ej=np.array([l[1] for l in L], np.int32),
                            Z=np.stack([l[2] for l in L]) if L else np.zeros((0, 7)), w=np.tile(self.w_loop, (len(L), 1)), K4=self.K4, bf=self.bf, huber=self.huber_delta))
        return out

    def optimize(self, vo, params=None, **kw):
        """every segment in one call.  Returns one (frame_ids, T_c_w) per segment; .last keeps per segment dict(lm_id, xyz (every landmark of the
        windows, moved), in_problem, problem, xyz_problem, stats, obs_chi2)."""
        ps = self.problems()
        off = lambda k: np.cumsum([0] + [len(p[k]) for p in ps]).astype(np.int32)
        cat = lambda k, shape, dt: np.concatenate([np.asarray(p[k], dt).reshape(shape) for p in ps]) if ps else np.zeros(shape, dt).reshape(shape)
        offsets = dict(kf=off("T"), lm=off("X"), obs=off("kf"), edge=off("ei"))
        out = vo.full_ba(cat("T", (-1, 7), np.float64), cat("X", (-1, 3), np.float64), offsets,
                         dict(kf=cat("kf", (-1,), np.int32), lm=cat("lm", (-1,), np.int32), uv=cat("uv", (-1, 2), np.float32), disp=cat("disp", (-1,), np.float32)),
                         dict(i=cat("ei", (-1,), np.int32), j=cat("ej", (-1,), np.int32), Z=cat("Z", (-1, 7), np.float64), w=cat("w", (-1, 6), np.float64)),
                         K4=self.K4, bf=self.bf, huber_delta=self.huber_delta, params=params, **kw)
        self.last, trajs = [], []
        for k, (s, p) in enumerate(zip(self.segs, ps)):
            T = out["T"][offsets["kf"][k]:offsets["kf"][k + 1]]; Xp = out["xyz"][offsets["lm"][k]:offsets["lm"][k + 1]]
            X = s["X_old"].copy()
            if len(X):
                c = s["carrier"]
                if len(s["ids"]):   # the landmarks outside the problem follow their keyframe's final correction
                    X = se3_act(se3_mul(se3_inverse(T[c]), s["T_old"][c]), X)
                X[s["part"]] = Xp
            self.last.append(dict(lm_id=s["lm_id"], xyz=X, in_problem=s["part"], problem=p, xyz_problem=Xp, stats=out["stats"][k],
                                  obs_chi2=out["obs_chi2"][offsets["obs"][k]:offsets["obs"][k + 1]]))
            ids_in = np.empty_like(s["ids"]); T_in = np.empty_like(T)   # (back in the order the trajectory came in)
            ids_in[s["order"]] = s["ids"]; T_in[s["order"]] = T
            trajs.append((ids_in, T_in))
        return trajs
