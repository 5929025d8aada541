"""GPU: several independent sequences in one batch (vslam_set_segments).  The contract is bit identity: for every segment, every output of every
entry point that takes "a batch of consecutive frames" equals what the same entry gives for a batch that holds that segment alone (frame indices
and offsets rebased).  So the yardstick of every case is the same library on each segment alone, without a table; the plain builder is also held
against oracle/windows.c per segment.  Random tables with the invariants of test_gpu_windows._random_tracks, kp capacity 64, ample capacities.

The layouts put boundaries where the 256-frame chunks of the scans, the 32-row staging of kf_set_kernel and its 64-frame band can go wrong.
Every case is guarded: the same concatenated tables through the same call WITHOUT a table must differ from the segmented result, otherwise the
case would show nothing.  No stage of these entries picks a kernel form by launch size, so nothing is pinned with vslam_set_tuning."""
import numpy as np
import pytest

from segments_ref import concat_windows, split_tables

pytestmark = pytest.mark.gpu

CAP = 64


def _many(seed=5, n=70):
    return np.concatenate([[0], np.cumsum(np.random.default_rng(seed).integers(1, 6, n))]).tolist()


LAYOUTS = {
    "chunk": [0, 255, 256, 258, 330],
    "span": [0, 3, 290, 291, 292, 330],      # a segment that spans frame 256 without starting on a chunk; adjacent one-frame segments
    "ones": [0, 1, 100, 101],
    "many": _many(),                          # 70 segments of 1 to 5 frames
}
LOST = {"chunk": 3, "span": 1, "ones": 1, "many": None}   # the segment that gets twelve rejections in a row (many: the first one long enough)


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {thr: pkg.VO(device=0, max_batch=1, pnp_reproj_thr=thr) for thr in (4.0, 300.0)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module")
def tables(oracle):
    """one set of random tables per layout (shared, never modified): the front-end tables, inlier counts that reject / track / accept, random
    absolute poses for the entries that take them, and a state vector with twelve rejections in a row inside one segment"""
    from test_gpu_windows import _random_tracks
    out = {}
    for li, (name, first) in enumerate(LAYOUTS.items()):
        rng = np.random.default_rng(40 + li)
        F = first[-1]
        kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = _random_tracks(rng, F, CAP, CAP)
        num_inl = rng.choice([0, 5, 40, 90, 150], F - 1, p=[0.1, 0.1, 0.4, 0.2, 0.2]).astype(np.int32)
        G = np.stack([oracle.se3_exp(np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 0.05, 3)])) for _ in range(F)])
        state = rng.choice([0, 1, 2], F, p=[0.3, 0.2, 0.5]).astype(np.int32)
        lens = np.diff(first)
        k = LOST[name] if LOST[name] is not None else int(np.flatnonzero(lens >= 5)[0])
        lo = first[k]
        if lens[k] >= 14:   # twelve rejections in a row: the segment ends Lost
            state[lo + 1:lo + 13] = 0; num_inl[lo:lo + 12] = 0
        num_inl[np.asarray(first[1:-1]) - 1] = 0   # (a boundary item's tables are arbitrary: as one sequence these frames would be rejected)
        out[name] = dict(kps=kps, lr=lr, nlr=nlr, xyz=xyz, valid=valid, rel=rel, f2f=f2f, nf2f=nf2f, inl=inl, T_rel=T_rel, nk=nk, num_inl=num_inl,
                         G=G, state=state, lost_seg=k if lens[k] >= 14 else None)
    return out


class _Dev:
    """the concatenated tables on the device, uploaded once; a segment's tables are the same buffers at a row offset"""

    def __init__(self, pkg, t):
        import torch
        self.pkg, self.torch = pkg, torch
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.F = len(t["kps"])
        self.t = {k: d(t[k].view(np.uint8) if t[k].dtype.fields else t[k]) for k in ("kps", "lr", "nlr", "xyz", "valid", "rel", "f2f", "nf2f", "inl", "T_rel", "nk",
                                                                                       "num_inl", "G", "state")}
        self.row = {k: (v[0].numel() * v.element_size() if v.dim() > 1 else v.element_size()) for k, v in self.t.items()}

    def ptr(self, k, lo):
        return self.t[k].data_ptr() + lo * self.row[k]

    def tracks(self, lo, hi):
        tr = self.pkg.TracksIn()
        tr.n_frames = hi - lo; tr.kp_capacity = CAP; tr.lr_capacity = CAP; tr.match_capacity = CAP; tr.pnp_capacity = CAP
        tr.d_kps = self.ptr("kps", lo); tr.d_lr = self.ptr("lr", lo); tr.d_nlr = self.ptr("nlr", lo); tr.d_xyz = self.ptr("xyz", lo)
        tr.d_valid = self.ptr("valid", lo); tr.d_reliable = self.ptr("rel", lo); tr.d_nkps = self.ptr("nk", lo)
        # (a one-frame batch has no pair: the pointers are not read, any valid address serves)
        tr.d_f2f = self.ptr("f2f", min(lo, self.F - 2)); tr.d_nf2f = self.ptr("nf2f", min(lo, self.F - 2)); tr.d_pose_inlier = self.ptr("inl", min(lo, self.F - 2))
        tr.d_T_rel = self.ptr("T_rel", min(lo, self.F - 2))
        return tr

    def windows(self, ctx, entry, lo, hi, n_kf, policy=0):
        """one builder call on frames [lo, hi) -> numpy dict in the key names of oracle.build_windows (+ kf_frame / evicted / state)"""
        torch, pkg = self.torch, self.pkg
        n = hi - lo
        lm_cap = e_cap = n * CAP * n_kf   # ample: a window holds at most n_kf x CAP landmarks, each seen at most once per frame
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        o = dict(lm_off=z(n + 1, torch.int32), edge_off=z(n + 1, torch.int32), n_kf=z(n, torch.int32), T=z((n, n_kf, 7), torch.float64),
                 xyz=z((lm_cap, 3), torch.float32), reliable=z(lm_cap, torch.uint8), lm_inlier=z(lm_cap, torch.uint8), kf_idx=z(e_cap, torch.int32),
                 lm_idx=z(e_cap, torch.int32), uv=z((e_cap, 2), torch.float32), status=z(1, torch.int32))
        bb = pkg.BaBatch()
        bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["edge_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
        bb.d_reliable = o["reliable"].data_ptr(); bb.d_lm_inlier = o["lm_inlier"].data_ptr(); bb.d_kf_idx = o["kf_idx"].data_ptr()
        bb.d_lm_idx = o["lm_idx"].data_ptr(); bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["n_kf"].data_ptr()
        tr = self.tracks(lo, hi)
        st = o["status"].data_ptr()
        if entry == "plain":
            ctx.build_windows_dev(tr, n_kf, lm_cap, e_cap, bb, st)
        else:
            o["kf_frame"] = z((n, n_kf), torch.int32); o["evicted"] = z(n, torch.int32)
            if entry == "kf":
                ctx.build_windows_kf_dev(tr, n_kf, policy, 0.5, lm_cap, e_cap, bb, o["kf_frame"].data_ptr(), o["evicted"].data_ptr(), st)
            else:
                o["state"] = z(n, torch.int32)
                ctx.build_windows_gated_dev(tr, n_kf, policy, 0.5, self.ptr("num_inl", min(lo, self.F - 2)), lm_cap, e_cap, bb, o["kf_frame"].data_ptr(),
                                            o["evicted"].data_ptr(), o["state"].data_ptr(), st)
        ctx.sync()
        g = {k: v.cpu().numpy() for k, v in o.items()}
        g["status"] = int(g["status"][0])
        return g


def _trim(w):
    """a whole-batch result in the shape concat_windows gives: per-landmark / per-edge arrays cut to the totals"""
    n = len(w["lm_off"]) - 1
    nl, ne = int(w["lm_off"][n]), int(w["edge_off"][n])
    out = dict(w)
    for k in ("xyz", "reliable", "lm_inlier"):
        out[k] = w[k][:nl]
    for k in ("kf_idx", "lm_idx", "uv"):
        out[k] = w[k][:ne]
    return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a if k in b)


def _segmented_vs_alone(ctx, dev, first, entry, n_kf, policy=0):
    """runs `entry` with the table, alone per segment and without a table on the concatenated tables; asserts table == alone, table != no table"""
    F = first[-1]
    ctx.set_segments(first)
    got = _trim(dev.windows(ctx, entry, 0, F, n_kf, policy))
    ctx.set_segments(None)
    alone = [dev.windows(ctx, entry, lo, hi, n_kf, policy) for lo, hi in zip(first[:-1], first[1:])]
    want = concat_windows(alone)
    assert got["status"] == want["status"] and sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (entry, policy, n_kf, k)
    plain = _trim(dev.windows(ctx, entry, 0, F, n_kf, policy))
    assert not _same(plain, got), "the case shows nothing: without a table the output is the same"
    return got, alone


@pytest.mark.parametrize("thr", [4.0, 300.0])
@pytest.mark.parametrize("n_kf", [1, 10, 12])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_builders_per_segment(pkg, oracle, ctxs, tables, layout, n_kf, thr):
    """vslam_build_windows_dev against per-segment calls of itself (array_equal after rebasing, poses included) and against oracle.build_windows per
    segment (the tolerances of test_gpu_windows: xyz rtol 3e-6 / atol 2e-5, poses rtol 1e-9 / atol 1e-11); vslam_build_windows_kf_dev with policy 1
    and vslam_build_windows_gated_dev with policies 0 and 1 against per-segment calls of themselves.  Track rule 1, the context's reprojection
    threshold at 4 and 300 px."""
    first, t = LAYOUTS[layout], tables[layout]
    ctx = ctxs[thr]
    ctx.set_tuning(track_rule=1)
    dev = _Dev(pkg, t)
    try:
        got, alone = _segmented_vs_alone(ctx, dev, first, "plain", n_kf)
        assert got["n_kf"].max() == min(n_kf, int(np.diff(first).max())) and (got["n_kf"][first[:-1]] == 1).all()
        parts = split_tables({k: t[k] for k in ("kps", "lr", "nlr", "xyz", "valid", "rel", "f2f", "nf2f", "inl", "T_rel")}, first)
        ws = [oracle.build_windows(p["kps"], p["lr"], p["nlr"], p["xyz"], p["valid"], p["rel"], p["f2f"], p["nf2f"], p["inl"], p["T_rel"], n_kf=n_kf,
                                   lm_capacity=len(p["kps"]) * CAP * n_kf, edge_capacity=len(p["kps"]) * CAP * n_kf, reproj_thr=thr, track_rule=1) for p in parts]
        w = concat_windows(ws)
        assert w["status"] == 0 and got["status"] == 0
        for k in ("lm_off", "edge_off", "n_kf", "kf_idx", "lm_idx", "uv", "reliable"):
            assert np.array_equal(got[k], w[k]), k
        assert np.allclose(got["xyz"], w["xyz"], rtol=3e-6, atol=2e-5), np.abs(got["xyz"] - w["xyz"]).max()
        assert np.allclose(got["T"], w["T"], rtol=1e-9, atol=1e-11)
        # the culled sets (policy 1) and the gated ones (policies 0 and 1)
        kf, _ = _segmented_vs_alone(ctx, dev, first, "kf", n_kf, 1)
        for lo, hi in zip(first[:-1], first[1:]):
            m = kf["kf_frame"][lo:hi]
            assert ((m == -1) | ((m >= lo) & (m < hi))).all() and m[0, 0] == lo
        for policy in (0, 1):
            g, _ = _segmented_vs_alone(ctx, dev, first, "gated", n_kf, policy)
            assert (g["state"][first[:-1]] == 2).all() and set(np.unique(g["state"])) == {0, 1, 2}
    finally:
        ctx.set_segments(None)


def _run(ctx, torch, fn, outs):
    fn(*[o.data_ptr() for o in outs])
    ctx.sync()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_chain_gate_and_pairs_per_segment(pkg, ctxs, tables, layout):
    """vslam_chain_poses_dev, vslam_gate_states_dev (both `absolute` values), vslam_frame_pairs_dev and vslam_gate_states_pairs_dev against
    per-segment calls.  One segment holds twelve rejections in a row: it ends Lost (pred -1, state 3) and the segment after it equals its lone run."""
    import torch
    first, t = LAYOUTS[layout], tables[layout]
    F = first[-1]
    ctx = ctxs[4.0]
    dev = _Dev(pkg, t)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    pp = lambda k, lo: dev.ptr(k, min(lo, F - 2))   # a per-pair table at a segment's first pair (a one-frame segment has none: not read)

    def calls(lo, hi, pred_in):
        n = hi - lo
        r = {}
        r["G"], = _run(ctx, torch, lambda o: ctx.chain_poses_dev(n, pp("T_rel", lo), o), [z((n, 7), torch.float64)])
        r["state_rel"], = _run(ctx, torch, lambda o: ctx.gate_states_dev(n, pp("T_rel", lo), 0, pp("num_inl", lo), o), [z(n, torch.int32)])
        r["state_abs"], = _run(ctx, torch, lambda o: ctx.gate_states_dev(n, dev.ptr("G", lo), 1, pp("num_inl", lo), o), [z(n, torch.int32)])
        gap = torch.full((max(n - 1, 1),), -9.0, dtype=torch.float64, device="cuda")
        r["pred"], r["gap"] = _run(ctx, torch, lambda p, g: ctx.frame_pairs_dev(n, dev.ptr("state", lo), p, g), [z(n, torch.int32), gap])
        r["gap"] = r["gap"][:n - 1]
        # the gate against a pairing: the pairing above, with a few entries moved back by one (still inside the frame's own segment)
        d_pred = torch.from_numpy(pred_in).cuda()
        r["state_pairs"], = _run(ctx, torch, lambda o: ctx.gate_states_pairs_dev(n, dev.ptr("G", lo), d_pred.data_ptr(), pp("num_inl", lo), o), [z(n, torch.int32)])
        return r

    try:
        # the pairing the gate is taken against: each frame's own predecessor f - 1, or f - 2 for every third frame where that stays in the segment
        start = np.repeat(first[:-1], np.diff(first))
        f = np.arange(F)
        pred_in = np.where(f == start, -1, np.where((f % 3 == 0) & (f - 2 >= start), f - 2, f - 1)).astype(np.int32)
        ctx.set_segments(first)
        got = calls(0, F, pred_in)
        ctx.set_segments(None)
        none = calls(0, F, pred_in)
        lone = [calls(lo, hi, np.where(pred_in[lo:hi] >= 0, pred_in[lo:hi] - lo, -1).astype(np.int32)) for lo, hi in zip(first[:-1], first[1:])]
        for k in ("G", "state_rel", "state_abs", "state_pairs"):
            assert np.array_equal(got[k], np.concatenate([r[k] for r in lone])), k
            assert not np.array_equal(got[k], none[k]), "%s: the case shows nothing" % k
        assert np.array_equal(got["pred"], np.concatenate([np.where(r["pred"] >= 0, r["pred"] + lo, -1) for r, lo in zip(lone, first)]))
        assert not np.array_equal(got["pred"], none["pred"])
        assert (got["pred"][first[:-1]] == -1).all() and (got["G"][first[:-1]] == np.array([0, 0, 0, 1, 0, 0, 0.0])).all()
        for r, lo, hi in zip(lone, first[:-1], first[1:]):
            assert np.array_equal(got["gap"][lo:hi - 1], r["gap"])
            if lo > 0:
                assert got["gap"][lo - 1] == 1.0   # the boundary item
            p = got["pred"][lo + 1:hi]
            assert ((p == -1) | ((p >= lo) & (p < hi))).all()
        k = t["lost_seg"]
        if k is not None:
            lo, hi = first[k], first[k + 1]
            # (frames lo + 1 .. lo + 12 are rejected: frame lo + 12 has eleven rejections between it and frame lo, so it is the first Lost one)
            assert (got["pred"][lo + 12:hi] == -1).all() and got["pred"][lo + 11] == lo and (got["state_pairs"][lo + 12:hi] == 3).all()
            assert (none["pred"][hi:] == -1).all()                     # one sequence: Lost is absorbing ...
            if k + 1 < len(first) - 1 and first[k + 2] - hi > 1:
                assert (got["pred"][hi + 1:first[k + 2]] >= hi).all()  # ... segments: the next one starts afresh
            assert (got["state_pairs"][first[k + 1:-1]] == 2).all()
        else:
            assert layout == "many"
    finally:
        ctx.set_segments(None)


def test_refusals_and_clearing(pkg, ctxs, tables):
    """a malformed table is refused and the old one survives; with a table set, a call of another n_frames or with a chunk input is refused;
    clearing the table restores the one-sequence output bit for bit"""
    import torch
    first, t = LAYOUTS["ones"], tables["ones"]
    F = first[-1]
    ctx = ctxs[4.0]
    dev = _Dev(pkg, t)
    try:
        before = _trim(dev.windows(ctx, "plain", 0, F, 10))
        fresh = pkg.VO(device=0, max_batch=1)   # (the shared contexts have held a table before: a context's buffers only grow)
        try:
            base_bytes = fresh.device_bytes
            fresh.set_segments(first)
            assert fresh.device_bytes > base_bytes   # the table is counted
        finally:
            fresh.close()
        ctx.set_segments(first)
        seg = _trim(dev.windows(ctx, "plain", 0, F, 10))
        assert not _same(seg, before)
        for bad, word in (([1, 5, F], "first[0]"), ([0, 5, 5, F], "ascend"), ([0, 7, 3, F], "ascend")):
            with pytest.raises(pkg.VslamError) as e:
                ctx.set_segments(bad)
            assert word in str(e.value), str(e.value)
        lib = pkg.load_library()
        assert lib.vslam_set_segments(ctx.h, 2, None) == pkg.VSLAM_ERR_ARG and lib.vslam_set_segments(ctx.h, -1, None) == pkg.VSLAM_ERR_ARG
        assert _same(_trim(dev.windows(ctx, "plain", 0, F, 10)), seg)   # the old table is still in place
        # another n_frames
        out = torch.zeros((F, 7), dtype=torch.float64, device="cuda")
        for call in (lambda: dev.windows(ctx, "plain", 0, F - 1, 10), lambda: dev.windows(ctx, "kf", 1, F, 10, 1), lambda: dev.windows(ctx, "gated", 0, 50, 10, 1),
                     lambda: ctx.chain_poses_dev(F - 1, dev.ptr("T_rel", 0), out.data_ptr()),
                     lambda: ctx.gate_states_dev(F + 1, dev.ptr("T_rel", 0), 0, dev.ptr("num_inl", 0), out.data_ptr()),
                     lambda: ctx.frame_pairs_dev(5, dev.ptr("state", 0), out.data_ptr(), out.data_ptr()),
                     lambda: ctx.gate_states_pairs_dev(F - 1, dev.ptr("G", 0), dev.ptr("state", 0), dev.ptr("num_inl", 0), out.data_ptr())):
            with pytest.raises(pkg.VslamError) as e:
                call()
            assert "segment table covers %d frames" % F in str(e.value), str(e.value)
        # chunk inputs
        carry = torch.zeros((CAP, 4), dtype=torch.float32, device="cuda")
        for field, val in (("d_T_abs", dev.ptr("G", 0)), ("d_carry_in", carry.data_ptr())):
            tr = dev.tracks(0, F)
            setattr(tr, field, val)
            bb = pkg.BaBatch()
            z = torch.zeros(F * CAP * 12, dtype=torch.float64, device="cuda")
            for name in ("d_lm_off", "d_edge_off", "d_T_c_w", "d_xyz", "d_reliable", "d_lm_inlier", "d_kf_idx", "d_lm_idx", "d_uv", "d_n_kf"):
                setattr(bb, name, z.data_ptr())
            with pytest.raises(pkg.VslamError) as e:
                ctx.build_windows_dev(tr, 10, F * CAP, F * CAP, bb, z.data_ptr())
            assert "chunk" in str(e.value), str(e.value)
        ctx.sync()
        ctx.set_segments(None)
        after = _trim(dev.windows(ctx, "plain", 0, F, 10))
        assert sorted(after) == sorted(before) and all(np.array_equal(after[k], before[k]) for k in before)
    finally:
        ctx.set_segments(None)


# ------------------------------------------------------------------------------------------------ the pipeline
SEGMENTS = (13, 1, 12)
NOISE_FRAME = 4   # of the 13-frame segment, as tests/test_gpu_recover.py plants its noise frames

# how every download() array is indexed: by image (left 0..B-1 | right 0..B-1), by frame, by frame holding batch frame indices, by frame pair
# (item i = the pair i -> i + 1; the item before a segment's first frame has no counterpart in the lone pipeline), by landmark, by edge
BY_IMAGE = ("cnt", "kps", "desc")
BY_FRAME = ("nlr", "lr", "xyz", "valid", "rel", "frame_state", "frame_state_prev", "map_feat", "map_nfeat", "T_c_w", "ba_T", "ba_nkf")
BY_FRAME_INDEX = ("ba_kf_frame", "ba_evicted", "map_pred")
BY_PAIR = ("nf2f", "pn", "ninl", "Tpnp", "f2f", "pxyz", "puv", "inl", "map_f2f", "map_nf2f", "map_n", "map_xyz", "map_uv", "map_index", "map_inl", "map_ninl",
           "map_gap")
BY_LM = ("ba_xyz", "ba_rel", "ba_inl")
BY_EDGE = ("ba_kf", "ba_lm", "ba_uv")
OTHER = ("ba_lm_off", "ba_e_off", "ba_build_status", "ba_chi2", "seg_first")


@pytest.fixture(scope="module")
def rendered(synth):
    """the three segments' sequences, rendered once (seed + 7919 s, the default of KeyframePipeline(segments=...)), and the 13-frame one with a
    noise frame planted"""
    seqs = [synth.stereo_sequence(max(2, n) if n > 1 else 1, seed=6 + 7919 * s) for s, n in enumerate(SEGMENTS)]
    noisy = list(seqs[0])
    noisy[NOISE_FRAME] = (synth.noise_image(100 + NOISE_FRAME), synth.noise_image(200 + NOISE_FRAME)) + tuple(noisy[NOISE_FRAME][2:])
    return seqs, [noisy] + seqs[1:]


def _pipeline_vs_lone(seqs, **kw):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = sum(SEGMENTS)
    first = np.concatenate([[0], np.cumsum(SEGMENTS)])
    common = dict(anms_num=500, unique_frames=B, seed=6, ba_windows="tracks", **kw)
    runs = []
    for args in [dict(B=B, segments=list(SEGMENTS), segment_sequences=seqs)] + [dict(B=n, sequence=seqs[s]) for s, n in enumerate(SEGMENTS)]:
        p = KeyframePipeline(**args, **common)
        try:
            p.step()
            out = p.download()
            assert (p.vo.ba_status(p.B) == 0).all()
            runs.append((out, p.trajectories() if "segments" in args else [p.trajectory()]))
        finally:
            p.close()
    (seg, seg_traj), lone = runs[0], runs[1:]
    assert np.array_equal(seg["seg_first"], first) and len(seg_traj) == len(SEGMENTS)
    classified = BY_IMAGE + BY_FRAME + BY_FRAME_INDEX + BY_PAIR + BY_LM + BY_EDGE + OTHER
    assert not [k for k in seg if k not in classified], [k for k in seg if k not in classified]
    status = 0
    for s, (lo, hi) in enumerate(zip(first[:-1], first[1:])):
        one, (one_traj,) = lone[s]
        n = hi - lo
        assert sorted(k for k in seg if k != "seg_first") == sorted(one), s
        for k in one:
            a, b = seg[k], one[k]
            if k in BY_IMAGE:
                ok = np.array_equal(a[lo:hi], b[:n]) and np.array_equal(a[B + lo:B + hi], b[n:])
            elif k in BY_FRAME:
                ok = np.array_equal(a[lo:hi], b)
            elif k in BY_FRAME_INDEX:
                ok = np.array_equal(a[lo:hi], np.where(b >= 0, b + lo, b))
            elif k in BY_PAIR:
                ok = np.array_equal(a[lo:hi - 1], b[:n - 1])
            elif k in BY_LM or k in BY_EDGE:
                off = seg["ba_lm_off" if k in BY_LM else "ba_e_off"]
                ok = np.array_equal(a[off[lo]:off[hi]], b[:off[hi] - off[lo]])
            elif k in ("ba_lm_off", "ba_e_off"):
                ok = np.array_equal(a[lo:hi + 1] - a[lo], b)
            else:
                ok = True
            assert ok, (s, k)
        status |= int(one["ba_build_status"][0])
        assert np.array_equal(seg_traj[s][0], one_traj[0]) and np.array_equal(seg_traj[s][1], one_traj[1]), s
        assert len(one_traj[0]) >= 1
    assert int(seg["ba_build_status"][0]) == status
    assert (seg["nf2f"][first[1:-1] - 1] == 0).all() and (seg["pn"][first[1:-1] - 1] == 0).all()
    assert seg["ba_e_off"][B] > seg["ba_lm_off"][B] > 1000   # real windows with tracks longer than one frame
    return seg, lone


def test_pipeline_segments_sliding(rendered):
    seg, _ = _pipeline_vs_lone(rendered[0])
    assert np.array_equal(seg["ba_nkf"], np.concatenate([np.minimum(np.arange(n) + 1, 10) for n in SEGMENTS]))


def test_pipeline_segments_reference_culling(rendered):
    _pipeline_vs_lone(rendered[0], window_policy="reference")


def test_pipeline_segments_gated_culling(rendered):
    seg, _ = _pipeline_vs_lone(rendered[0], keyframe_gate=True, window_policy="reference")
    assert (seg["frame_state"][[0, 13, 14]] == 2).all()


def test_pipeline_segments_map_passes(rendered):
    seg, _ = _pipeline_vs_lone(rendered[0], pose_inputs="map", pose_passes=3)
    assert (seg["T_c_w"][[0, 13, 14]] == np.array([0, 0, 0, 1, 0, 0, 0.0])).all() and (seg["map_n"][[12, 13]] == 0).all()


def test_pipeline_segments_full_reference_mode(rendered):
    """RANSAC, map inputs, the gate inside the passes, the reference's query set, its failure handling and its culling, three passes, with one noise
    frame in the 13-frame segment: that frame is rejected there and nowhere else does anything change"""
    seg, lone = _pipeline_vs_lone(rendered[1], pose="ransac", pose_inputs="map", keyframe_gate="per_pass", f2f_queries="features", rejected_frames="recover",
                                  window_policy="reference", pose_passes=3)
    assert seg["frame_state"][NOISE_FRAME] == 0 and seg["map_pred"][NOISE_FRAME + 1] == NOISE_FRAME - 1 and seg["map_gap"][NOISE_FRAME] == 2.0
    assert (seg["map_pred"][[0, 13, 14]] == -1).all() and (seg["map_nf2f"][[12, 13]] == 0).all()


def test_pipeline_one_segment_is_the_plain_pipeline(rendered):
    """segments=[B] equals the pipeline without the argument"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    seq = rendered[0][2]
    outs = []
    for kw in (dict(segments=[12], segment_sequences=[seq]), dict(sequence=seq)):
        p = KeyframePipeline(12, anms_num=500, unique_frames=12, seed=6, ba_windows="tracks", window_policy="reference", **kw)
        try:
            p.step()
            outs.append((p.download(), p.trajectories()))
        finally:
            p.close()
    (a, ta), (b, tb) = outs
    assert sorted(k for k in a if k != "seg_first") == sorted(b)
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert len(ta) == len(tb) == 1 and np.array_equal(ta[0][0], tb[0][0]) and np.array_equal(ta[0][1], tb[0][1])
