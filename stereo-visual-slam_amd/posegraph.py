"""Host side of the pose-graph stage: trajectories and loop-closure edges in, corrected trajectories out (include/vslam_hip.h "pose-graph
optimisation").  PoseGraph only lays the arrays out; the optimisation is VO.optimize_pose_graph, one persistent workgroup per sequence on the device."""
import numpy as np


def _rot(T):
    x, y, z, w = T[..., 0], T[..., 1], T[..., 2], T[..., 3]
    R = np.empty(T.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def se3_mul(A, B):
    """A o B for poses stored as quaternion x, y, z, w then translation (csrc/se3_device.h), over the leading axis"""
    ax, ay, az, aw = (A[..., k] for k in range(4)); bx, by, bz, bw = (B[..., k] for k in range(4))
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz], -1)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([q, np.einsum("...ij,...j->...i", _rot(A), B[..., 4:]) + A[..., 4:]], -1)


def se3_inverse(A):
    q = A[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([q, -np.einsum("...ji,...j->...i", _rot(A), A[..., 4:])], -1)


def se3_log(T):
    """Sophus' SE3 log (csrc/se3_device.h): tangent [upsilon; omega] of poses (n, 7)"""
    v, w = T[..., :3], T[..., 3]
    sq = (v * v).sum(-1); n = np.sqrt(sq)
    ns = np.where(n < 1e-10, 1.0, n); ws = np.where(np.abs(w) < 1e-10, 1.0, w)
    two_atan = np.where(n < 1e-10, 2.0 / ws - 2.0 * sq / ws ** 3, np.where(np.abs(w) < 1e-10, np.where(w > 0, np.pi, -np.pi) / ns, 2.0 * np.arctan(n / ws) / ns))
    om = two_atan[..., None] * v
    th = two_atan * n; small = np.abs(th) < 1e-10
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0, (1.0 - ths * np.cos(0.5 * ths) / (2.0 * np.sin(0.5 * ths))) / (ths * ths))
    O = np.zeros(T.shape[:-1] + (3, 3))
    O[..., 0, 1] = -om[..., 2]; O[..., 0, 2] = om[..., 1]; O[..., 1, 0] = om[..., 2]
    O[..., 1, 2] = -om[..., 0]; O[..., 2, 0] = -om[..., 1]; O[..., 2, 1] = om[..., 0]
    Vi = np.eye(3) - 0.5 * O + c[..., None, None] * (O @ O)
    return np.concatenate([np.einsum("...ij,...j->...i", Vi, T[..., 4:]), om], -1)


class PoseGraph:
    """One graph per sequence: the nodes are a trajectory's frames in ascending frame order, consecutive nodes are tied by an odometry edge
    Z = T_{k+1} T_k^-1 taken from the trajectory itself, and accepted loop-closure rows (LOOP_EDGE_DTYPE, KeyframePipeline.loop_closures) add the
    edges that correct it.  Node 0 of every sequence is held.

    motion_limit: an odometry edge is left out (and counted in .report["odometry_dropped"]) when |log Z| > motion_limit x its frame gap -- the
    limit of VO::check_motion_estimation (visual_odometry.cpp:329, 5.0), the rule the library already judges a tracked pose by.  A pose the tracker
    got across a cut in the recording is not a measurement; left in, it outweighs every loop edge and, at residuals of a radian and a hundred
    metres, Levenberg-Marquardt does not converge on it.  The chain is then broken there, which the device entry takes as a result.  None keeps all.

    w_odo / w_loop: the diagonal information of an odometry / a loop edge as a pair (translation, rotation).  Both default to 1.0, which says only
    that a metre and a radian weigh the same and a loop edge as much as an odometry edge: NO MEASURED DEFAULT EXISTS -- neither the tracker's nor
    the RANSAC pose stage's covariance has been measured.  A caller who knows them should pass their inverses.

    Limits: one workgroup per graph, so a single 4096-node graph uses one compute unit.  Steps of one drive shown through show_sequence each start a
    world of their own; a graph across steps needs poses the caller has put into one world.  BA landmarks are not moved (fullba.FullBA does that)."""

    def __init__(self, w_odo=(1.0, 1.0), w_loop=(1.0, 1.0), motion_limit=5.0):
        self.w_odo = np.repeat(np.asarray(w_odo, np.float64), 3); self.w_loop = np.repeat(np.asarray(w_loop, np.float64), 3)
        assert self.w_odo.shape == (6,) and self.w_loop.shape == (6,)
        self.seqs = []        # [seq key, frame_ids (ascending), T (n, 7)] in the order they were added
        self.loops = []       # (sequence index, node q, node c, T_q_c)
        self.motion_limit = None if motion_limit is None else float(motion_limit)
        self.report = dict(added=0, not_accepted=0, unknown_seq=0, unknown_frame=0, odometry_dropped=0)
        self.last = None      # the result of the most recent optimize(): dict(stats, edge_chi2, is_loop, rejected)

    def add_trajectory(self, seq, frame_ids, T_c_w):
        """the frames of sequence `seq` (any hashable key; the `seq` of the loop rows) with their poses, in any order"""
        assert all(s[0] != seq for s in self.seqs), "sequence %r added twice" % (seq,)
        ids = np.asarray(frame_ids, np.int64); T = np.asarray(T_c_w, np.float64).reshape(-1, 7)
        assert len(ids) == len(T) and len(np.unique(ids)) == len(ids)
        o = np.argsort(ids, kind="stable")
        self.seqs.append([seq, ids[o], T[o].copy()])

    def add_loop_edges(self, rows):
        """the ACCEPTED rows of a LOOP_EDGE_DTYPE array whose two frames are nodes of their sequence become edges (i = frame_q, j = frame_c,
        Z = T_q_c).  Returns, and adds up in .report, what happened to every row: added, not_accepted, unknown_seq, unknown_frame."""
        rep = dict(added=0, not_accepted=0, unknown_seq=0, unknown_frame=0)
        keys = [s[0] for s in self.seqs]
        for row in rows:
            if not row["accepted"]:
                rep["not_accepted"] += 1
                continue
            if int(row["seq"]) not in keys:
                rep["unknown_seq"] += 1
                continue
            s = keys.index(int(row["seq"]))
            ids = self.seqs[s][1]
            q, c = np.searchsorted(ids, int(row["frame_q"])), np.searchsorted(ids, int(row["frame_c"]))
            if q >= len(ids) or c >= len(ids) or ids[q] != row["frame_q"] or ids[c] != row["frame_c"] or q == c:
                rep["unknown_frame"] += 1
                continue
            self.loops.append((s, int(q), int(c), np.array(row["T_q_c"], np.float64)))
            rep["added"] += 1
        for k, v in rep.items():
            self.report[k] += v
        return rep

    def arrays(self):
        """(T, node_off, edges dict(off, i, j, Z, w), is_loop, loop_index): the batch VO.optimize_pose_graph takes; every graph's odometry edges come
        first, then its loop edges in the order they were added (loop_index: their positions in .loops)"""
        node_off = np.cumsum([0] + [len(s[1]) for s in self.seqs]).astype(np.int32)
        ei, ej, Z, w, is_loop, loop_index, edge_off, dropped = [], [], [], [], [], [], [0], 0
        for s, (_, ids, T) in enumerate(self.seqs):
            n = len(ids)
            n_odo = 0
            if n > 1:
                Zo = se3_mul(T[1:], se3_inverse(T[:-1]))
                keep = np.ones(n - 1, bool)
                if self.motion_limit is not None:
                    keep = ~(np.linalg.norm(se3_log(Zo), axis=-1) > self.motion_limit * np.diff(ids))
                n_odo = int(keep.sum()); dropped += n - 1 - n_odo
                ei.append(np.arange(1, n)[keep]); ej.append(np.arange(0, n - 1)[keep]); Z.append(Zo[keep])
                w.append(np.tile(self.w_odo, (n_odo, 1))); is_loop.append(np.zeros(n_odo, bool)); loop_index.append(np.full(n_odo, -1))
            mine = [k for k, l in enumerate(self.loops) if l[0] == s]
            if mine:
                ei.append(np.array([self.loops[k][1] for k in mine])); ej.append(np.array([self.loops[k][2] for k in mine]))
                Z.append(np.stack([self.loops[k][3] for k in mine])); w.append(np.tile(self.w_loop, (len(mine), 1)))
                is_loop.append(np.ones(len(mine), bool)); loop_index.append(np.array(mine))
            edge_off.append(edge_off[-1] + n_odo + len(mine))
        self.report["odometry_dropped"] = dropped
        cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt).reshape(shape) if parts else np.zeros(shape, dt).reshape(shape)
        edges = dict(off=np.array(edge_off, np.int32), i=cat(ei, (-1,), np.int32), j=cat(ej, (-1,), np.int32), Z=cat(Z, (-1, 7), np.float64),
                     w=cat(w, (-1, 6), np.float64))
        T = cat([s[2] for s in self.seqs], (-1, 7), np.float64)
        return T, node_off, edges, cat(is_loop, (-1,), bool), cat(loop_index, (-1,), np.int64)

    def optimize(self, vo, reject_chi2=None, params=None, **kw):
        """One pass over every sequence in one call.  With reject_chi2 the library's own idiom follows -- optimise, classify by chi2, optimise again:
        the loop edges whose chi2 after the first pass exceeds reject_chi2 are switched off and a second pass runs FROM THE INPUT POSES without them
        (no robust kernel: a gross false edge bends the first pass too far to start from it).  Returns one (frame_ids, T_c_w) per sequence, in the
        order they were added: the shape KeyframePipeline.trajectories() returns, so write_trajectory takes it.  .last keeps dict(stats, edge_chi2,
        is_loop, rejected = indices into .loops of the edges the second pass left out, first_pass = the first pass's stats and chi2 when there were
        two)."""
        T, node_off, edges, is_loop, loop_index = self.arrays()
        out = vo.optimize_pose_graph(T, node_off, edges, params=params, **kw)
        last = dict(stats=out["stats"], edge_chi2=out["edge_chi2"], is_loop=is_loop, rejected=np.zeros(0, np.int64))
        if reject_chi2 is not None:
            flag = is_loop & (out["edge_chi2"] > float(reject_chi2))
            if flag.any():
                first = dict(stats=out["stats"], edge_chi2=out["edge_chi2"])
                out = vo.optimize_pose_graph(T, node_off, edges, active=(~flag).astype(np.uint8), params=params, **kw)
                last = dict(stats=out["stats"], edge_chi2=out["edge_chi2"], is_loop=is_loop, rejected=loop_index[flag], first_pass=first)
        self.last = last
        return [(s[1].copy(), out["T"][node_off[k]:node_off[k + 1]].copy()) for k, s in enumerate(self.seqs)]
