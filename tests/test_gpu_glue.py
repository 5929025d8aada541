"""GPU: the glue kernels between the matcher and the pose stage on their own -- gather_uv_kernel (vslam_gather_matched_uv_dev) and
build_pnp_inputs_kernel (vslam_build_pnp_inputs_dev) -- against the plain loops of tests/glue_ref.py.  Both only copy, so every comparison is on
bytes.  The tables are not what a rendered scene gives: counts at, around and above their capacities and below zero, indices out of range on
either side, an L/R table with repeated queryIdx, survivors spread unevenly over the four waves of more than one 256-match round, and an output
capacity below the number of survivors.  Every output buffer is poisoned first; what the rule does not write must still hold the poison.

B = 6 items per call, kp_capacity 300, match_capacity 700 (three rounds, the last one partial), lr_capacity 300."""
import numpy as np
import pytest

import glue_ref as R

pytestmark = pytest.mark.gpu

B, KP, MC, LRC = 6, 300, 700, 300
BAD = (-1, KP, -2 ** 31, 2 ** 31 - 1, -7, KP + 5)       # indices outside [0, KP)
P_XYZ, P_UV, P_N, P_K = -777.25, -555.5, -99, -77        # the poison of each output


def _item(pkg, rng, survive, nm, nlr=None, dup=False):
    """the tables of one item whose frame-to-frame match i survives iff survive[i] (i < 700; matches past the item's count are filled the same way,
    so a kernel that ignores the count shows).  dup: some keypoints occur twice or three times in the L/R table, with different points and
    validity, so the result depends on which occurrence the table keeps."""
    cur = np.zeros(KP, pkg.KEYPOINT_DTYPE)
    cur["x"] = rng.uniform(0, 1241, KP).astype(np.float32); cur["y"] = rng.uniform(0, 376, KP).astype(np.float32)
    lr = np.zeros(LRC, pkg.DMATCH_DTYPE)
    perm = rng.permutation(KP)
    n_lr = 280 if nlr is None else nlr                    # rows the rule reads: min(n_lr, LRC), never negative here
    used = max(min(n_lr, LRC), 0)
    lr["queryIdx"] = np.concatenate([perm[:260], rng.choice(BAD, LRC - 260)])   # 260 distinct keypoints, then out-of-range rows
    lr["trainIdx"] = rng.integers(0, KP, LRC)
    valid = (rng.random(LRC) < 0.7).astype(np.uint8)
    if dup:                                               # rows 200..259 repeat the keypoints of rows 0..59, rows 240..259 also those of 100..119
        lr["queryIdx"][200:260] = lr["queryIdx"][0:60]
        lr["queryIdx"][100:120] = lr["queryIdx"][40:60]
        valid[0:60] = (np.arange(60) % 2).astype(np.uint8); valid[200:260] = ((np.arange(60) // 2) % 2).astype(np.uint8)
        valid[100:120] = 1
    xyz = rng.uniform(-50, 50, (LRC, 3)).astype(np.float32)
    # the reference's table decides which keypoints can survive
    kp2lr = np.full(KP, -1, np.int64)
    for i in range(used):
        q = int(lr["queryIdx"][i])
        if 0 <= q < KP:
            kp2lr[q] = i
    good = np.array([k for k in range(KP) if kp2lr[k] >= 0 and valid[kp2lr[k]]], np.int64)
    no_lr = np.array([k for k in range(KP) if kp2lr[k] < 0], np.int64)
    inval = np.array([k for k in range(KP) if kp2lr[k] >= 0 and not valid[kp2lr[k]]], np.int64)
    pick = lambda pool, i: int(rng.choice(pool)) if len(pool) else int(BAD[i % len(BAD)])
    f2f = np.zeros(MC, pkg.DMATCH_DTYPE)
    for i in range(MC):
        t = int(rng.integers(0, KP))
        if survive[i] and len(good):
            q = int(rng.choice(good))
        elif i % 4 == 0:                                  # the ways a match is dropped, in rotation: a keypoint without an L/R match,
            q = pick(no_lr, i)
        elif i % 4 == 1:                                  # one whose L/R match is invalid,
            q = pick(inval, i)
        elif i % 4 == 2:                                  # a queryIdx out of range,
            q = int(BAD[(i // 4) % len(BAD)])
        else:                                             # a trainIdx out of range
            q = pick(good, i); t = int(BAD[(i // 4) % len(BAD)])
        f2f["queryIdx"][i] = q; f2f["trainIdx"][i] = t
    rows = max(min(nm, MC), 0)
    return dict(cur=cur, lr=lr, nlr=n_lr, valid=valid, xyz=xyz, f2f=f2f, nm=nm, survivors=int(survive[:rows].sum()) if len(good) else 0)


def _patterns():
    i = np.arange(MC)
    return dict(none=np.zeros(MC, bool), all=np.ones(MC, bool), third=i % 3 == 0,
                # every survivor in the last wave of round 0 and the first wave of round 1
                waves=((i >= 192) & (i < 256)) | ((i >= 256) & (i < 320)),
                # waves 0..3 of every round carry 1, 13, 37 and 64 survivors
                skew=np.isin(i % 256, np.concatenate([[5], 64 + np.arange(13) * 3, 128 + np.arange(37), 192 + np.arange(64)])))


@pytest.fixture(scope="module")
def batches(pkg):
    """name -> list of B items; shared, never modified"""
    rng = np.random.default_rng(2024)
    p = _patterns()
    mk = lambda pat, nm, **kw: _item(pkg, rng, p[pat], nm, **kw)
    return {
        # the issue's counts, every third match surviving
        "counts": [mk("third", n) for n in (0, 1, 255, 256, 257, 700)],
        # a count above the capacity, a negative one, and the survivor patterns at the full table
        "patterns": [mk("all", 900), mk("all", -3), mk("none", 700), mk("waves", 700), mk("skew", 700), mk("third", 700, dup=True)],
        # the same patterns at counts that end inside a round, L/R counts above capacity, zero and negative, duplicates again
        "ragged": [mk("waves", 257), mk("skew", 255), mk("all", 256, nlr=900), mk("all", 700, nlr=0), mk("third", 700, nlr=-3), mk("skew", 700, dup=True)],
    }


def _reference(items, out_cap):
    return [R.build_pnp_inputs(it["f2f"], it["nm"], MC, it["lr"], it["nlr"], LRC, it["xyz"], it["valid"], it["cur"], out_cap) for it in items]


def test_patterns_are_what_they_claim(batches):
    """the reference's survivor counts of the constructed items (CPU arithmetic only; here so that the GPU cases below mean what they say)"""
    n = {name: [w[1] for w in _reference(items, MC)] for name, items in batches.items()}
    for name, items in batches.items():
        assert n[name] == [it["survivors"] for it in items], name     # the intended pattern, cut at the item's count
    assert n["counts"] == [0, 1, 85, 86, 86, 234]
    assert n["patterns"] == [700, 0, 0, 128, 2 * (1 + 13 + 37 + 64) + 1 + 13 + 37, 234]     # (round 2 ends at lane 187: nothing of wave 3)
    assert n["ragged"] == [65, 1 + 13 + 37 + 63, 256, 0, 0, 2 * 115 + 51]


def _up(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


@pytest.mark.parametrize("out_cap", [700, 100])
@pytest.mark.parametrize("name", ["counts", "patterns", "ragged"])
def test_build_pnp_inputs(vo, pkg, batches, name, out_cap):
    """d_nout exact, the first d_nout rows and d_kp2lr byte-equal to the reference, every later row still poisoned, a second call the same bytes.
    At out_capacity 100 the cut is exact too: a survivor written at slot == out_capacity would land in row 0 of the NEXT item's block, and in
    "patterns" the item after the fully surviving one has a negative count, so its row 0 must still hold the poison."""
    import torch
    items = batches[name]
    want = _reference(items, out_cap)
    st = lambda k: np.stack([it[k] for it in items])
    d = dict(f2f=_up(torch, st("f2f")), nm=_up(torch, np.array([it["nm"] for it in items], np.int32)), lr=_up(torch, st("lr")),
             nlr=_up(torch, np.array([it["nlr"] for it in items], np.int32)), xyz=_up(torch, st("xyz")), valid=_up(torch, st("valid")),
             cur=_up(torch, st("cur")))
    o = dict(kp2lr=torch.full((B, KP), P_K, dtype=torch.int32, device="cuda"), xyz=torch.full((B, out_cap, 3), P_XYZ, dtype=torch.float32, device="cuda"),
             uv=torch.full((B, out_cap, 2), P_UV, dtype=torch.float32, device="cuda"), n=torch.full((B,), P_N, dtype=torch.int32, device="cuda"))

    def call():
        torch.cuda.synchronize()
        vo.build_pnp_inputs_dev(d["f2f"].data_ptr(), d["nm"].data_ptr(), MC, d["lr"].data_ptr(), d["nlr"].data_ptr(), LRC, d["xyz"].data_ptr(),
                                d["valid"].data_ptr(), d["cur"].data_ptr(), KP, B, o["kp2lr"].data_ptr(), o["xyz"].data_ptr(), o["uv"].data_ptr(),
                                o["n"].data_ptr(), out_cap)
        vo.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    got = call()
    assert got["n"].tolist() == [w[1] for w in want]
    assert out_cap == MC or any(it["survivors"] > out_cap for it in items)    # the small capacity cuts at least one item of every batch
    for b, (kp2lr, nout, xyz, uv) in enumerate(want):
        assert np.array_equal(got["kp2lr"][b], kp2lr), (name, b)
        assert got["xyz"][b, :nout].tobytes() == xyz.tobytes(), (name, b)
        assert got["uv"][b, :nout].tobytes() == uv.tobytes(), (name, b)
        assert (got["xyz"][b, nout:] == np.float32(P_XYZ)).all() and (got["uv"][b, nout:] == np.float32(P_UV)).all(), (name, b)
    again = call()    # the same buffers, not poisoned again
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_duplicate_query_needs_last_wins(batches):
    """the duplicated-queryIdx items are cases at all.  The kernel fills the table with `for (i = tid; i < nlr; i += 256)`: rows i and i + 200 of one
    keypoint (i < 56) are handled in the same trip by threads i and i + 200, lanes of waves 0 and 3.  With a plain store `kp2lr[q] = i` nothing
    orders the two writes, so the table may keep the FIRST occurrence; atomicMax keeps the larger index whatever the order.  Here: keeping the
    first occurrence changes the reference's table on at least 60 keypoints, changes the validity of at least 10 of them, and the item's matches
    query those -- so with the plain store at least one possible lane order disagrees with test_build_pnp_inputs.  CPU arithmetic only."""
    for name in ("patterns", "ragged"):
        it = batches[name][5]
        last = R.build_pnp_inputs(it["f2f"], it["nm"], MC, it["lr"], it["nlr"], LRC, it["xyz"], it["valid"], it["cur"], MC)
        kp2lr_first = np.full(KP, -1, np.int32)
        for i in reversed(range(min(it["nlr"], LRC))):     # first wins == last wins on the table walked backwards
            q = int(it["lr"]["queryIdx"][i])
            if 0 <= q < KP:
                kp2lr_first[q] = i
        assert (kp2lr_first != last[0]).sum() >= 60
        changed = [k for k in np.flatnonzero(kp2lr_first != last[0]) if it["valid"][kp2lr_first[k]] != it["valid"][last[0][k]]]
        assert len(changed) >= 10 and np.isin(it["f2f"]["queryIdx"][:it["nm"]], changed).any()


def test_gather_matched_uv(vo, pkg):
    """counts 0, 1, 256, 257, above the capacity and negative; indices out of range on both sides in both columns (clamped, glue_ref.gather_uv);
    rows at or past the count keep the poison"""
    import torch
    rng = np.random.default_rng(77)
    counts = [0, 1, 256, 257, 900, -3]
    kq = np.zeros((B, KP), pkg.KEYPOINT_DTYPE); kt = np.zeros((B, KP), pkg.KEYPOINT_DTYPE)
    for k in (kq, kt):
        k["x"] = rng.uniform(0, 1241, (B, KP)).astype(np.float32); k["y"] = rng.uniform(0, 376, (B, KP)).astype(np.float32)
    m = np.zeros((B, MC), pkg.DMATCH_DTYPE)
    m["queryIdx"] = rng.integers(0, KP, (B, MC)); m["trainIdx"] = rng.integers(0, KP, (B, MC))
    bad = rng.random((B, MC))
    m["queryIdx"][bad < 0.15] = rng.choice(BAD, int((bad < 0.15).sum()))
    m["trainIdx"][bad > 0.85] = rng.choice(BAD, int((bad > 0.85).sum()))
    m["queryIdx"][:, 0] = -1; m["trainIdx"][:, 0] = KP      # (the one row of the count-1 item is out of range on both sides)
    d_kq, d_kt, d_m, d_n = _up(torch, kq), _up(torch, kt), _up(torch, m), _up(torch, np.array(counts, np.int32))
    uq = torch.full((B, MC, 2), P_UV, dtype=torch.float32, device="cuda"); ut = torch.full((B, MC, 2), P_XYZ, dtype=torch.float32, device="cuda")

    def call():
        torch.cuda.synchronize()
        vo.gather_matched_uv_dev(d_kq.data_ptr(), d_kt.data_ptr(), KP, d_m.data_ptr(), d_n.data_ptr(), MC, B, uq.data_ptr(), ut.data_ptr())
        vo.sync()
        return uq.cpu().numpy(), ut.cpu().numpy()

    gq, gt = call()
    for b, n in enumerate(counts):
        rows, wq, wt = R.gather_uv(kq[b], kt[b], m[b], n, MC)
        assert rows == max(min(n, MC), 0)
        assert gq[b, :rows].tobytes() == wq.tobytes() and gt[b, :rows].tobytes() == wt.tobytes(), b
        assert (gq[b, rows:] == np.float32(P_UV)).all() and (gt[b, rows:] == np.float32(P_XYZ)).all(), b
    aq, at = call()
    assert aq.tobytes() == gq.tobytes() and at.tobytes() == gt.tobytes()
