"""The train-nearest kernel on FP4 matrix instructions with an f32 key (dot + tie-break fraction): the cases the random matcher tests reach only by luck,
against oracle/match.c, and (no GPU needed) the f32 key arithmetic against integer keys.

The kernel's key for query row i inside the tiles tile0 .. tile1 - 1 of a workgroup is dot + (32 tile1 - 1 - i) * 2^-12, formed as
C = (31 - i % 32) * 2^-12 handed to the first matrix instruction of each 32-row tile plus 32 * 2^-12 added to the running maximum before every tile; rows past nq in the
last tile get C = -2^22.  Largest key = smallest distance, then smallest row -- the first-minimum rule of the integer key (dot << 16 | 0xFFFF - i) it replaces."""
import numpy as np
import pytest

f32 = np.float32
UNIT = f32(1.0 / 4096.0)
NO_ROW = f32(-4194304.0)


# ---------------------------------------------------------------------------------------------- the key model (CPU)
def _fold_f32(dots, tile0, tile1):
    """the kernel's fold in float32 arithmetic: dots[i] for the nq rows; returns (dot, row) decoded from the running maximum over tiles tile0 .. tile1 - 1"""
    nq = len(dots)
    m = f32(-np.inf)
    lr = np.arange(32)
    for tile in range(tile0, tile1):
        rows = tile * 32 + lr
        c = ((31 - lr).astype(f32) * UNIT).astype(f32)
        c[rows >= nq] = NO_ROW
        d = np.zeros(32, f32); ok = rows < nq; d[ok] = dots[rows[ok]]      # (a padded row repeats a real descriptor in the kernel; its dot is immaterial)
        keys = (c + d).astype(f32)                                       # the matrix instruction's accumulator: C + the sum of +-1 products, exact
        m = f32(m + f32(32.0) * UNIT)
        m = max(m, keys.max())
    fl = np.floor(m)
    return int(fl), 32 * tile1 - 1 - int((m - fl) * f32(4096.0))


def _fold_int(dots, tile0, tile1):
    lo, hi = tile0 * 32, min(len(dots), tile1 * 32)
    keys = (dots[lo:hi].astype(np.int64) << 16) + (0xFFFF - np.arange(lo, hi))
    k = int(keys.max())
    return k >> 16, 0xFFFF - (k & 0xFFFF)


def test_f32_key_model_is_the_integer_key():
    # every (dot, row) pair of a 4096-row item (all 513 integers in [-256, 256]; the 257 even ones are the dots 256 - 2 hamming): the key as the fold carries it to the end (C of its tile, then 32 * 2^-12 per later tile, each step
    # rounded to float32) equals dot + (4095 - row) / 4096 exactly, so float order == integer key order, and it decodes to the pair
    dot = np.arange(-256, 257, dtype=np.int64)[:, None]
    row = np.arange(4096, dtype=np.int64)[None, :]
    key = (dot.astype(f32) + ((31 - row % 32).astype(f32) * UNIT)).astype(f32)
    key = np.broadcast_to(key, (513, 4096)).copy()
    later = 127 - row // 32                                               # tiles folded after the row's own
    for step in range(1, 128):
        key = np.where(later >= step, (key + f32(32.0) * UNIT).astype(f32), key)
    assert key.dtype == np.float32
    assert np.array_equal(key.astype(np.float64) * 4096.0, (dot * 4096 + (4095 - row)).astype(np.float64))
    fl = np.floor(key)
    assert np.array_equal(fl.astype(np.int64), np.broadcast_to(dot, key.shape))
    assert np.array_equal(4095 - ((key - fl) * f32(4096.0)).astype(np.int64), np.broadcast_to(row, key.shape))
    # a row that does not compete stays below every real key, whatever its dot and however many tiles follow
    assert f32(256.0) + NO_ROW + f32(4096.0) * UNIT < f32(-256.0)
    # random items through the running-maximum form, whole and split into query ranges like the kernel's qsplit, with heavy ties
    rng = np.random.default_rng(5)
    for case in range(2000):
        nq = int(rng.integers(1, 4097)) if case % 4 else int(rng.choice([1, 31, 32, 33, 4064, 4095, 4096]))
        kind = case % 3
        if kind == 0:
            dots = rng.integers(-128, 129, nq) * 2
        elif kind == 1:
            dots = np.full(nq, int(rng.integers(-128, 129)) * 2)          # all tied: row 0 of the range wins
        else:
            dots = np.full(nq, -200); dots[rng.integers(0, nq, 5)] = 180  # few tied winners scattered over the tiles
        dots = dots.astype(np.int64)
        ntiles = (nq + 31) // 32
        qsplit = int(rng.choice([1, 2, 4, 16]))
        per = (ntiles + qsplit - 1) // qsplit
        for split in range(qsplit):
            t0, t1 = split * per, min(ntiles, split * per + per)
            if t0 < t1:
                assert _fold_f32(dots, t0, t1) == _fold_int(dots, t0, t1), (case, nq, split)


# ---------------------------------------------------------------------------------------------- the kernel (GPU)
def _same(got, want, tag=None):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in ("queryIdx", "trainIdx", "distance"):
        assert np.array_equal(got[f], want[f]), (tag, f)


def _run(vo, pkg, qs, ts, cap, gate=0, sels=None):
    """one batched device call (the subset entry when sels is given); returns the DMATCH array of every item"""
    import torch
    B = len(qs)
    dev = torch.device("cuda:0")
    Q = np.zeros((B, cap, 32), np.uint8); T = np.zeros((B, cap, 32), np.uint8)
    for b in range(B):
        Q[b, :len(qs[b])] = qs[b]; T[b, :len(ts[b])] = ts[b]
    dq, dt = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev)
    dnq = torch.tensor([len(q) for q in qs], dtype=torch.int32, device=dev); dnt = torch.tensor([len(t) for t in ts], dtype=torch.int32, device=dev)
    dgap = torch.ones(B, dtype=torch.float64, device=dev)
    dout = torch.zeros((B, cap, 16), dtype=torch.uint8, device=dev); dn = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if sels is None:
        vo.feature_matching_dev(dq.data_ptr(), cap * 32, dnq.data_ptr(), dt.data_ptr(), cap * 32, dnt.data_ptr(), dgap.data_ptr(), gate, B, cap,
                                dout.data_ptr(), cap, dn.data_ptr())
    else:
        S = np.full((B, cap), -1, np.int32)
        for b in range(B):
            S[b, :len(sels[b])] = sels[b]
        ds = torch.from_numpy(S).to(dev); dns = torch.tensor([len(s) for s in sels], dtype=torch.int32, device=dev)
        vo.feature_matching_subset_dev(dq.data_ptr(), cap * 32, dnq.data_ptr(), ds.data_ptr(), dns.data_ptr(), cap, dt.data_ptr(), cap * 32,
                                       dnt.data_ptr(), dgap.data_ptr(), gate, B, cap, dout.data_ptr(), cap, dn.data_ptr())
    vo.sync()
    out, n = dout.cpu().numpy(), dn.cpu().numpy()
    return [out[b].reshape(-1).view(pkg.DMATCH_DTYPE)[:n[b]].copy() for b in range(B)]


def _want(oracle, q, t, gate=0, sel=None):
    if sel is not None:
        sel = np.asarray(sel, np.int64)
        if len(sel) == 0:
            return np.zeros(0, oracle.DMATCH_DTYPE)
        q = np.ascontiguousarray(q[sel])
    m = (oracle.feature_matching(q, t, 1.0) if gate else oracle.bf_match_xcheck(q, t)).copy()
    if sel is not None:
        m["queryIdx"] = sel[m["queryIdx"]]
    return m


def _flip(d, bit):
    d = d.copy(); d[bit // 8] ^= np.uint8(1 << (bit % 8)); return d


@pytest.fixture(scope="module")
def big(pkg):
    """a context for batches that fill the chip without splitting the query range (2 column blocks x 512 items of capacity 1024)"""
    ctx = pkg.VO(params=pkg.default_params(max_batch=512), device=0)
    yield ctx
    ctx.close()


def _last_row_items():
    """4096 query rows: (a) the only near row of column 5 is row 4095; (b) rows 0 and 4095 tie for column 7 (row 0 wins); (c) rows 4064 and 4095 tie in the last tile"""
    rng = np.random.default_rng(31)
    items = []
    for kind in range(3):
        q = rng.integers(0, 256, (4096, 32), dtype=np.uint8); t = rng.integers(0, 256, (777, 32), dtype=np.uint8)
        if kind == 0:
            q[4095] = t[5]
        elif kind == 1:
            q[0] = _flip(t[7], 3); q[4095] = _flip(t[7], 200)
        else:
            q[4064] = _flip(t[9], 17); q[4095] = _flip(t[9], 17)
        items.append((q, t))
    return items


@pytest.mark.gpu
def test_row_4095_wins_and_ties_with_row_0(vo, pkg, oracle):
    items = _last_row_items()
    for k, (q, t) in enumerate(items):
        want = _want(oracle, q, t)
        col = {0: 5, 1: 7, 2: 9}[k]; row = {0: 4095, 1: 0, 2: 4064}[k]
        assert want["queryIdx"][want["trainIdx"] == col].tolist() == [row]      # the oracle agrees with the construction
        _same(vo.feature_matching(q, t, 1.0, gate=False), want, ("host", k))  # one item: the query range is split over workgroups
        _same(vo.feature_matching(q, t, 1.0, gate=True), _want(oracle, q, t, 1), ("host gated", k))
    # the three items in one device call of capacity 4096
    got = _run(vo, pkg, [q for q, _ in items], [t for _, t in items], 4096)
    for k, (q, t) in enumerate(items):
        _same(got[k], _want(oracle, q, t), ("dev", k))


@pytest.mark.gpu
def test_every_residue_of_nq_and_nt(big, pkg, oracle, synth):
    """512 items of capacity 1024 (query range not split): nt = 513 .. 1024 takes every residue mod 512, so every one mod 128 (a wave's columns) and
    mod 32 (a column tile); nq = 1 .. 224 takes every residue mod 32 sixteen times, over one to seven tiles; then nt = 1 .. 512 with nq the other way round"""
    for base in (513, 1):
        qs, ts = [], []
        for k in range(512):
            nt = base + k
            nq = 1 + (k if base == 513 else 511 - k) % 32 + 32 * ((k // 32) % 7)
            q, t = synth.random_descriptors(nq, nt, seed=9000 + base + k)
            qs.append(q); ts.append(t)
        assert {len(q) % 32 for q in qs} == set(range(32)) and {len(t) % 512 for t in ts} == set(range(512))
        got = _run(big, pkg, qs, ts, 1024)
        for k in range(512):
            _same(got[k], _want(oracle, qs[k], ts[k]), (base, k))


@pytest.mark.gpu
def test_distances_0_and_256(vo, pkg, oracle):
    rng = np.random.default_rng(33)
    t = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    q[3] = t[10]; q[150] = t[10]; q[77] = ~t[20]; q[199] = t[299]; q[0] = ~t[0]
    want = _want(oracle, q, t)
    assert 0.0 in want["distance"]
    _same(vo.feature_matching(q, t, 1.0, gate=False), want, "mixed")
    # every pair at distance 256, every pair at distance 0: all keys tie, row 0 takes column 0 and nothing else matches
    for nq, nt in ((40, 40), (100, 33), (33, 700)):
        z = np.zeros((nq, 32), np.uint8); o = np.full((nt, 32), 255, np.uint8)
        for a, b, d in ((z, o, 256.0), (z, np.zeros_like(o), 0.0)):
            want = _want(oracle, a, b)
            assert len(want) == 1 and want["distance"][0] == d
            _same(vo.feature_matching(a, b, 1.0, gate=False), want, (nq, nt, d))
            _same(_run(vo, pkg, [a], [b], 1024)[0], want, ("dev", nq, nt, d))


def _tied_item(rng, nq, nt, col, rows, dist_bits=(1,)):
    """all of `rows` sit at the same small distance from train column `col`, every other query row is random (distance ~128)"""
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8); t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for n, r in enumerate(rows):
        d = t[col]
        for b in dist_bits:
            d = _flip(d, (b + 13 * n) % 256)                            # different bits per row: equal distances, different descriptors
        q[r] = d
    return q, t


# local row lr of a 32-row tile lives in lane half (lr >> 2) & 1 of the accumulator layout
_TIES = [((37, 70, 130, 40), 37),      # tiles 1, 2, 4, 1; halves 1, 1, 0, 0: the winner is in half 1, a later row of its own tile in half 0
         ((33, 36), 33),               # one tile, half 0 before half 1
         ((36, 41), 36),               # one tile, half 1 before half 0
         ((95, 96), 95),               # last row of a tile (half 1) against the first of the next (half 0)
         ((4, 480, 517), 4),           # first tile against the last ones
         ((516, 485), 485)]


@pytest.mark.gpu
def test_tied_minima_across_tiles_and_lane_halves(vo, big, pkg, oracle):
    rng = np.random.default_rng(34)
    items = [_tied_item(rng, 520, 300 + 41 * k, 100 + k, rows, (1, 90)) for k, (rows, _) in enumerate(_TIES)]
    for k, (q, t) in enumerate(items):
        want = _want(oracle, q, t)
        assert want["queryIdx"][want["trainIdx"] == 100 + k].tolist() == [_TIES[k][1]]
        _same(vo.feature_matching(q, t, 1.0, gate=False), want, ("host", k))
    qs, ts = [q for q, _ in items], [t for _, t in items]
    # device calls: four items alone (query range split) and all six repeated to a batch of 512 (one workgroup per column block)
    for ctx, tag, n in ((vo, "split", 4), (big, "whole", 512)):
        got = _run(ctx, pkg, (qs * 86)[:n], (ts * 86)[:n], 1024)
        for k in range(min(n, 12)):
            _same(got[k], _want(oracle, qs[k % 6], ts[k % 6]), (tag, k))


@pytest.mark.gpu
def test_the_same_cases_through_the_subset_call(vo, pkg, oracle):
    """full, half and one-row selections: the key carries the RANK in the list, so the tie rule and the last-row cases move with the list"""
    rng = np.random.default_rng(35)
    qs, ts, sels = [], [], []
    q, t = _last_row_items()[1]                                            # rows 0 and 4095 tie for column 7
    for sel in (np.arange(4096), np.arange(1, 4096, 2), np.array([4095]), np.arange(0, 4096, 2)):
        qs.append(q); ts.append(t); sels.append(sel)
    got = _run(vo, pkg, qs, ts, 4096, 0, sels)
    for k in range(4):
        want = _want(oracle, qs[k], ts[k], 0, sels[k])
        _same(got[k], want, ("last rows", k))
    winners = [int(g["queryIdx"][g["trainIdx"] == 7][0]) for g in got]
    assert winners == [0, 4095, 4095, 0]
    qs, ts, sels = [], [], []
    for k, (rows, _) in enumerate(_TIES[:4]):
        q, t = _tied_item(rng, 520, 333, 50, rows)
        half = np.sort(np.unique(np.concatenate([rng.permutation(520)[:260], np.asarray(rows[1:], np.int64)])))   # drops the first tied row, maybe
        for sel in (np.arange(520), half, np.array([rows[-1]])):
            qs.append(q); ts.append(t); sels.append(sel)
    for lo in range(0, len(qs), 4):
        got = _run(vo, pkg, qs[lo:lo + 4], ts[lo:lo + 4], 1024, 1, sels[lo:lo + 4])
        for k in range(len(got)):
            _same(got[k], _want(oracle, qs[lo + k], ts[lo + k], 1, sels[lo + k]), ("ties", lo + k))
    # distances 0 and 256 through a selection
    z = np.zeros((64, 32), np.uint8); o = np.full((90, 32), 255, np.uint8)
    for sel in (np.arange(64), np.arange(32, 64), np.array([63])):
        for tt in (o, np.zeros_like(o)):
            _same(_run(vo, pkg, [z], [tt], 1024, 0, [sel])[0], _want(oracle, z, tt, 0, sel), ("0/256", len(sel)))


@pytest.mark.gpu
def test_split_query_range_equals_the_whole_one(vo, big, pkg, oracle, synth):
    """one small item alone (the query range split over up to 16 workgroups per column block, merged by atomicMin on the final key) against the same
    item inside a batch of 512 (one workgroup per column block, plain store): identical matches, both equal to the oracle's"""
    rng = np.random.default_rng(36)
    for nq, nt, seed in ((500, 500, 1), (1024, 1024, 2), (33, 1000, 3), (1000, 33, 4), (513, 129, 5)):
        q, t = synth.random_descriptors(nq, nt, seed=seed)
        q = q.copy(); src = rng.permutation(nq)[:nq // 3]; q[rng.permutation(nq)[:len(src)]] = q[src]      # duplicated query rows: ties
        for gate in (0, 1):
            want = _want(oracle, q, t, gate)
            alone = _run(vo, pkg, [q], [t], 1024, gate)[0]
            fill = synth.random_descriptors(64, 64, seed=99)
            batch = _run(big, pkg, [fill[0]] * 200 + [q] + [fill[0]] * 311, [fill[1]] * 200 + [t] + [fill[1]] * 311, 1024, gate)[200]
            _same(alone, want, ("alone", nq, nt, gate)); _same(batch, want, ("batch", nq, nt, gate))
            assert alone.tobytes() == batch.tobytes()
