"""Host side of match by projection (include/vslam_hip.h "match by projection"): which landmarks are projected into which keyframes after a step,
and what the matches mean for the map.  Reobserve only lays arrays out and reads results -- numpy, once per step, like fullba.py; the matching is
one vslam_project_match_dev call, handed in as a callable so that the yardstick (tests/project_match_ref.py) can stand in for the device.

Per segment, from what FullBA reads: the unique window landmarks, each at the position the last window left, descriptor row = identity (creating
frame x kp_capacity + creating keypoint) into the step's descriptor array.
LOCAL ITEMS.  For the keyframe at position p of the trajectory: the landmarks with an observation in a keyframe at positions p - neighbours ..
p + neighbours and none in p, at p's trajectory pose.
LOOP ITEMS.  For every accepted loop edge (q, c) between keyframes of the segment: the landmarks observed within loop_neighbours positions of c and
not in q go into q at T_q_c o T_c_w(c); the reverse direction into c at T_q_c^-1 o T_c_w(q).  Both in the old world: no pose-graph result is needed.
OWNERSHIP.  (frame, keypoint) -> landmark id: the creating observations (the id says it), and the windows' other observations found by their pixel
among the frame's keypoints (the first keypoint with that pixel; ambiguous and missing ones are counted).
APPLYING.  The MATCHED results sorted by (dist, frame, id) are applied greedily under one rule: a landmark class has at most one keypoint per frame.
A result either adds an observation or, when its keypoint is owned by another class, merges the two classes (union-find, canonical = the smallest
id); one that would break the rule is counted and dropped.
MERGE GATE (optional, the pipeline sets it).  Two landmarks are one world point only if their positions agree where they meet: the projected
landmark taken into the target frame by its item's pose and the keypoint's owner taken there by the frame's trajectory pose must lie within the
search radius of each other in u, in v and in the stereo disparity bf / z (the third row the full BA measures), both in front of the camera.  A
merge that fails is counted (refused_merge_position) and dropped: a fused class starts the full BA from ONE member's position, and a class fused
across different depths on one viewing ray would start behind some of its cameras."""
import numpy as np

from .posegraph import se3_inverse, se3_mul

KIND_LOCAL, KIND_LOOP = 0, 1
REOBS_DTYPE = np.dtype([("frame", "<i4"), ("lm_id", "<i8"), ("kp", "<i4"), ("u", "<f4"), ("v", "<f4"), ("dist", "<i4"), ("kind", "u1")])
PM_MATCHED = 0


class Reobserve:
    def __init__(self, kp_capacity, neighbours=10, loop_neighbours=2):
        self.cap = int(kp_capacity); self.neighbours = int(neighbours); self.loop_neighbours = int(loop_neighbours)
        assert self.neighbours >= 0 and self.loop_neighbours >= 0
        self.segs = []
        self.report = dict(landmarks=0, items_local=0, items_loop=0, projected_local=0, projected_loop=0, edges_used=0, edges_not_accepted=0, edges_unknown_seq=0,
                           edges_unknown_frame=0)

    def add_segment(self, first_frame, frame_ids, T, obs_frame, obs_lm_id, obs_uv, lm_id, lm_xyz):
        """as FullBA.add_segment: the segment's trajectory (frame ids local to the segment, poses T_c_w), the windows' observations as (batch frame,
        landmark id, uv) and landmarks as (id, world position), duplicates included, in window order"""
        ids = np.asarray(frame_ids, np.int64); order = np.argsort(ids, kind="stable")
        ids = ids[order]; T = np.asarray(T, np.float64).reshape(-1, 7)[order]
        N = len(ids)
        obs_frame = np.asarray(obs_frame, np.int64); obs_lm_id = np.asarray(obs_lm_id, np.int64); obs_uv = np.asarray(obs_uv, np.float32).reshape(-1, 2)
        lm_id = np.asarray(lm_id, np.int64); lm_xyz = np.asarray(lm_xyz, np.float64).reshape(-1, 3)
        uid, last = np.unique(lm_id[::-1], return_index=True)
        X = lm_xyz[::-1][last] if len(uid) else np.zeros((0, 3))
        key = obs_frame * (np.int64(1) << 40) + obs_lm_id
        _, firsts = np.unique(key, return_index=True)
        firsts.sort()
        of, ol, ouv = obs_frame[firsts] - int(first_frame), obs_lm_id[firsts], obs_uv[firsts]
        node = np.minimum(np.searchsorted(ids, of), max(N - 1, 0))
        known = (ids[node] == of) if N else np.zeros(len(of), bool)
        lidx = np.minimum(np.searchsorted(uid, ol), max(len(uid) - 1, 0))
        known &= (uid[lidx] == ol) if len(uid) else False
        node, lidx, ouv = node[known], lidx[known], ouv[known]
        by_pos = [np.unique(lidx[node == p]) for p in range(N)]
        self.report["landmarks"] += len(uid)
        self.segs.append(dict(first_frame=int(first_frame), ids=ids, T=T, lm_id=uid, X=X, obs_node=node, obs_lidx=lidx, obs_uv=ouv, by_pos=by_pos, loops=[]))

    def add_loop_edges(self, rows, frame_offset=0):
        """the ACCEPTED rows whose two frames (batch-wide + frame_offset) are keyframes of one segment; every row is counted in .report (FullBA's rule)"""
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
            rep["edges_used"] += 1

    def _near(self, s, p, reach, target):
        """the landmarks observed at positions p - reach .. p + reach of segment s and not at position `target`"""
        lo, hi = max(p - reach, 0), min(p + reach, len(s["ids"]) - 1)
        seen = np.unique(np.concatenate(s["by_pos"][lo:hi + 1])) if hi >= lo else np.zeros(0, np.int64)
        return np.setdiff1d(seen, s["by_pos"][target], assume_unique=True)

    def items(self):
        """the batch for vslam_project_match_dev, items sorted by image: dict(lm_off, item_img, item_T, lm_xyz, lm_desc_row) and, for apply(),
        item_kind, item_seg, lm_lidx.  Empty items are left out."""
        its = []   # (image, kind, segment, pose, landmark indices)
        for k, s in enumerate(self.segs):
            for p in range(len(s["ids"])):
                l = self._near(s, p, self.neighbours, p)
                if len(l):
                    its.append((s["first_frame"] + int(s["ids"][p]), KIND_LOCAL, k, s["T"][p], l))
            for q, c, T_q_c in s["loops"]:
                for into, frm, T_rel in ((q, c, T_q_c), (c, q, se3_inverse(T_q_c))):
                    l = self._near(s, frm, self.loop_neighbours, into)
                    if len(l):
                        its.append((s["first_frame"] + int(s["ids"][into]), KIND_LOOP, k, se3_mul(T_rel, s["T"][frm]), l))
        its.sort(key=lambda t: (t[0], t[1]))   # (stable: by image, local before loop)
        for t in its:
            self.report["items_local" if t[1] == KIND_LOCAL else "items_loop"] += 1
            self.report["projected_local" if t[1] == KIND_LOCAL else "projected_loop"] += len(t[4])
        n = [len(t[4]) for t in its]
        cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)
        self.batch = dict(lm_off=np.cumsum([0] + n).astype(np.int32), item_img=np.array([t[0] for t in its], np.int32),
                          item_T=np.array([t[3] for t in its], np.float64).reshape(-1, 7),
                          lm_xyz=cat([self.segs[t[2]]["X"][t[4]] for t in its], (0, 3), np.float64),
                          lm_desc_row=cat([self.segs[t[2]]["lm_id"][t[4]] for t in its], (0,), np.int32),
                          item_kind=np.array([t[1] for t in its], np.uint8), item_seg=np.array([t[2] for t in its], np.int32),
                          lm_lidx=cat([t[4] for t in its], (0,), np.int64))
        return self.batch

    def ownership(self, kps_xy, n):
        """(frame, keypoint) -> landmark id of the windows' observations, and per landmark class its frames: the creating observations directly, the
        others by their pixel among the frame's first n[frame] keypoints.  An observation whose keypoint is not found still occupies its frame."""
        rep = self.report
        rep.update(owned_creating=0, owned_by_pixel=0, pixel_ambiguous=0, pixel_not_found=0, ownership_conflicts=0)
        owner, frames = {}, {}
        kps_xy = np.asarray(kps_xy, np.float32)
        for s in self.segs:
            f_of = s["first_frame"] + s["ids"][s["obs_node"]]
            for f, l, uv in zip(f_of.tolist(), s["obs_lidx"].tolist(), s["obs_uv"]):
                lid = int(s["lm_id"][l])
                if lid // self.cap == f:
                    kp = lid % self.cap; rep["owned_creating"] += 1
                else:
                    nf = min(max(int(n[f]), 0), kps_xy.shape[1])
                    hit = np.flatnonzero((kps_xy[f, :nf, 0] == uv[0]) & (kps_xy[f, :nf, 1] == uv[1]))
                    if len(hit) == 0:
                        rep["pixel_not_found"] += 1; kp = -1
                    else:
                        kp = int(hit[0]); rep["owned_by_pixel"] += 1; rep["pixel_ambiguous"] += int(len(hit) > 1)
                frames.setdefault(lid, {})[f] = kp
                if kp >= 0:
                    if (f, kp) in owner and owner[(f, kp)] != lid:
                        rep["ownership_conflicts"] += 1
                    else:
                        owner[(f, kp)] = lid
        return owner, frames

    def _agree(self, gate, seg, T_item, X, f, own):
        """the merge gate: landmark position X under T_item against landmark `own` of segment `seg` under frame f's trajectory pose"""
        from .fullba import se3_act
        K4, bf, r = gate["K4"], float(gate["bf"]), float(gate["radius"])
        s = self.segs[seg]
        pos = int(np.searchsorted(s["ids"], f - s["first_frame"])); l = int(np.searchsorted(s["lm_id"], own))
        if pos >= len(s["ids"]) or s["ids"][pos] != f - s["first_frame"] or l >= len(s["lm_id"]) or s["lm_id"][l] != own:
            return False
        Pa, Pb = se3_act(np.asarray(T_item, np.float64), np.asarray(X, np.float64)), se3_act(s["T"][pos], s["X"][l])
        if not (Pa[2] > 0 and Pb[2] > 0):
            return False
        a = (K4[0] * Pa[0] / Pa[2], K4[1] * Pa[1] / Pa[2], bf / Pa[2]); c = (K4[0] * Pb[0] / Pb[2], K4[1] * Pb[1] / Pb[2], bf / Pb[2])
        return all(abs(x - y) <= r for x, y in zip(a, c))

    def apply(self, result, kps_xy, n, gate=None):
        """result: dict(match, dist, status) per landmark of items(); kps_xy (B, cap, 2) and n (B): the step's left keypoints.  Returns
        dict(observations (REOBS_DTYPE), merge = (ids, canonical) over the members of every class of two or more, merging_matches (REOBS_DTYPE: the
        matches that fused two classes; they add no observation of their own), report).  gate: dict(K4, bf, radius) switches the merge gate on."""
        b, rep = self.batch, self.report
        owner, frames = self.ownership(kps_xy, n)
        status = np.asarray(result["status"]); match = np.asarray(result["match"]); dist = np.asarray(result["dist"])
        item_of = np.repeat(np.arange(len(b["item_img"])), np.diff(b["lm_off"]))
        hit = np.flatnonzero(status == PM_MATCHED)
        for kind, name in ((KIND_LOCAL, "matched_local"), (KIND_LOOP, "matched_loop")):
            rep[name] = int((b["item_kind"][item_of[hit]] == kind).sum())
        lid_of = b["lm_desc_row"].astype(np.int64)
        fr = b["item_img"][item_of[hit]].astype(np.int64)
        hit = hit[np.lexsort((lid_of[hit], fr, dist[hit]))]   # by (dist, frame, id)
        parent = {}

        def find(a):
            r = a
            while parent.get(r, r) != r:
                r = parent[r]
            while parent.get(a, a) != a:
                parent[a], a = r, parent[a]
            return r

        rep.update(observations_added=0, observations_added_loop=0, merges=0, merges_loop=0, already_observed=0, refused_frame_taken=0, refused_merge_conflict=0,
                   refused_merge_position=0)
        rows, fused = [], []
        for i in hit.tolist():
            it = int(item_of[i]); f = int(b["item_img"][it]); kind = int(b["item_kind"][it]); lid = int(lid_of[i]); kp = int(match[i])
            c = find(lid)
            fc = frames.setdefault(c, {})
            own = owner.get((f, kp))
            if own is None:
                if f in fc:   # the class has a keypoint in this frame already (perhaps one that was not found among the keypoints)
                    rep["already_observed" if fc[f] == kp else "refused_frame_taken"] += 1
                    continue
                fc[f] = kp; owner[(f, kp)] = lid
                rows.append((f, lid, kp, kps_xy[f, kp, 0], kps_xy[f, kp, 1], int(dist[i]), kind))
                rep["observations_added"] += 1; rep["observations_added_loop"] += int(kind == KIND_LOOP)
                continue
            c2 = find(own)
            if c2 == c:
                rep["already_observed"] += 1
                continue
            f2 = frames.setdefault(c2, {})
            if any(g in f2 and (f2[g] != k or k < 0) for g, k in fc.items()):   # (an unknown keypoint equals none)
                rep["refused_merge_conflict"] += 1
                continue
            if gate is not None and not self._agree(gate, int(b["item_seg"][it]), b["item_T"][it], b["lm_xyz"][i], f, own):
                rep["refused_merge_position"] += 1
                continue
            lo_, hi_ = min(c, c2), max(c, c2)
            parent[hi_] = lo_
            merged = dict(frames.pop(hi_)); merged.update(frames[lo_]); frames[lo_] = merged
            rep["merges"] += 1; rep["merges_loop"] += int(kind == KIND_LOOP)
            fused.append((f, lid, kp, kps_xy[f, kp, 0], kps_xy[f, kp, 1], int(dist[i]), kind))
        members = sorted(a for a in parent if find(a) != a)
        roots = sorted({find(a) for a in members})
        ids = np.array(sorted(set(members) | set(roots)), np.int64)
        canonical = np.array([find(int(a)) for a in ids], np.int64)
        pack = lambda rs: np.array(rs, REOBS_DTYPE) if rs else np.zeros(0, REOBS_DTYPE)
        return dict(observations=pack(rows), merge=(ids, canonical), merging_matches=pack(fused), report=dict(rep))


def reobserve(segments, edges, kp_capacity, matcher, kps_xy, n, neighbours=10, loop_neighbours=2, frame_offset=0, merge_gate=None):
    """segments: one tuple of Reobserve.add_segment's arguments per segment; matcher(batch) -> dict(match, dist, status) for the batch items() lays
    out (all items in one call); merge_gate: Reobserve.apply's gate.  Returns what Reobserve.apply returns, with the Reobserve under "state"."""
    ro = Reobserve(kp_capacity, neighbours=neighbours, loop_neighbours=loop_neighbours)
    for seg in segments:
        ro.add_segment(*seg)
    if edges is not None:
        ro.add_loop_edges(edges, frame_offset=frame_offset)
    batch = ro.items()
    if len(batch["item_img"]):
        result = matcher(batch)
    else:
        result = dict(match=np.zeros(0, np.int32), dist=np.zeros(0, np.int32), status=np.zeros(0, np.uint8))
    out = ro.apply(result, kps_xy, n, gate=merge_gate)
    out["state"] = ro
    return out
