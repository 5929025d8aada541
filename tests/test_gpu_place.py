"""GPU: the place database -- add, score, select, verify -- bit for bit against tests/place_ref.py (all integer), the refused arguments, and the
verification against the three existing entries called by hand and against the oracle's matcher + RANSAC."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import place_ref as P

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _refusals(lib, err, section):
    """no(key, rc): the call returned `err` and left the message tests/golden/refused_messages.json holds under `key` -- the text the library gave
    before its host tier was put in order, which every later library must reproduce"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refused_messages.json")) as f:
        want = json.load(f)[section]

    def no(key, rc):
        assert rc == err, key
        assert lib.vslam_last_error().decode() == want[key], key
    return no


def _add(vo, db, descs, seqs, frames, add=None, ns=None, geom=None, kp_cap=None):
    """one vslam_place_add_dev call on items of numpy descriptor rows; geom = (kps list, xyz list, valid list) for a database with geometry"""
    import torch
    B = len(descs)
    cap = max(max((len(d) for d in descs), default=1), 1)
    D = np.zeros((B, cap, 32), np.uint8)
    for b, d in enumerate(descs):
        D[b, :len(d)] = d
    ns = [len(d) for d in descs] if ns is None else ns
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(_dev())
    dD, dn, ds, df = t(D, np.uint8), t(ns, np.int32), t(seqs, np.int32), t(frames, np.int32)
    da = None if add is None else t(add, np.int32)
    dk = dx = dv = None
    kp_cap = cap if kp_cap is None else kp_cap
    if geom is not None:
        import stereo_visual_slam_amd as pkg
        K = np.zeros((B, kp_cap), pkg.KEYPOINT_DTYPE); X = np.zeros((B, kp_cap, 3), np.float32); V = np.zeros((B, kp_cap), np.uint8)
        for b in range(B):
            m = min(len(geom[0][b]), kp_cap)
            K[b, :m]["x"] = geom[0][b][:m, 0]; K[b, :m]["y"] = geom[0][b][:m, 1]; X[b, :m] = geom[1][b][:m]; V[b, :m] = geom[2][b][:m]
        dk = torch.from_numpy(K.view(np.uint8).reshape(B, -1)).to(_dev()); dx = t(X, np.float32); dv = t(V, np.uint8)
    torch.cuda.synchronize()
    ptr = lambda a: None if a is None else a.data_ptr()
    return vo.place_add_dev(db, dD.data_ptr(), cap * 32, dn.data_ptr(), ptr(da), ds.data_ptr(), df.data_ptr(), ptr(dk), ptr(dx), ptr(dv), kp_cap, B)


def _score(vo, db, q0, nq, tau, min_gap, ld=None, sentinel=-77):
    import torch
    n = len(db)
    ld = n if ld is None else ld
    d = torch.full((nq, ld), sentinel, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    vo.place_score_dev(db, q0, nq, tau, min_gap, d.data_ptr(), ld)
    vo.sync()
    return d.cpu().numpy()


def _entries(synth, rng, ns, n_base=97):
    """descriptor blocks that share rows of one base set (each taken row with 0..12 flipped bits: inside and outside tau = 30 after two hops) plus
    random rows; duplicated rows inside every block of four rows or more"""
    base, _ = synth.random_descriptors(n_base, n_base, seed=int(rng.integers(1 << 30)))
    out = []
    for n in ns:
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        take = rng.permutation(n)[:(2 * n + 2) // 3]
        src = rng.integers(0, n_base, len(take))
        d[take] = base[src]
        for k in take:
            for _ in range(int(rng.integers(0, 13))):
                d[k, int(rng.integers(32))] ^= np.uint8(1 << int(rng.integers(8)))
        if n >= 4:
            d[rng.integers(0, n, n // 4)] = d[rng.integers(0, n, n // 4)]   # duplicate rows
        out.append(d)
    return out


@pytest.fixture(scope="module")
def shapes_db(vo, synth):
    """R = 97; entries with n in {0, 1, 31, 32, 33, 64, 97} and one of 120 rows (clamped), two sequences interleaved, added by two calls"""
    rng = np.random.default_rng(9)
    ns = [33, 0, 97, 1, 64, 31, 32, 120, 97, 33, 1, 64]
    descs = _entries(synth, rng, ns)
    seqs = [e % 2 for e in range(len(ns))]; frames = list(range(len(ns)))
    db = vo.place_db(rows=97, capacity=16, with_geometry=False)
    ref = P.PlaceRef(97, 16)
    assert _add(vo, db, descs[:5], seqs[:5], frames[:5]) == 0 == ref.add(descs[:5], ns[:5], seqs[:5], frames[:5])
    assert _add(vo, db, descs[5:], seqs[5:], frames[5:]) == 5 == ref.add(descs[5:], ns[5:], seqs[5:], frames[5:])
    yield db, ref
    db.close()


@pytest.mark.parametrize("tau,min_gap", [(30, 2), (12, 0), (60, 4)])
def test_score_shapes_sequences_and_two_adds(vo, shapes_db, tau, min_gap):
    db, ref = shapes_db
    n = len(ref)
    assert len(db) == n == 12 and [len(d) for d in ref.desc][7] == 97
    want = ref.score(0, n, tau, min_gap)
    got = _score(vo, db, 0, n, tau, min_gap)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (want >= 0).sum() > 10 and want.max() > 5 and (want == 0).any()
    # two sequences interleaved: an entry of the other sequence is never eligible
    assert (want[np.arange(n)[:, None] % 2 != np.arange(n)[None, :] % 2] == -1).all()
    # a query range that starts past the first add, a row stride above the entry count (the columns beyond keep their sentinel), and the same call twice
    got2 = _score(vo, db, 5, 7, tau, min_gap, ld=n + 5)
    assert np.array_equal(got2[:, :n], want[5:]) and (got2[:, n:] == -77).all()
    assert got2.tobytes() == _score(vo, db, 5, 7, tau, min_gap, ld=n + 5).tobytes()


def _bits(k, ones=False):
    """32 bytes with the first k bits set (ones: all set but the first k)"""
    b = np.zeros(256, np.uint8); b[:k] = 1
    if ones:
        b = 1 - b
    return np.packbits(b, bitorder="little")


@pytest.mark.parametrize("tau", [0, 30, 127, 128, 255])
@pytest.mark.parametrize("copies", [1, 33])
def test_score_tau_boundary(vo, tau, copies):
    """a planted pair at distance exactly tau (counts) and one at tau + 1 (does not), as single rows and as 33 duplicates of the row (two tiles)"""
    zero, one = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    rep = lambda d: np.repeat(d[None], copies, axis=0)
    descs = [rep(_bits(tau)), rep(_bits(tau + 1, ones=True)), rep(zero), rep(one)]   # d(zero, A) = tau, d(one, B) = tau + 1
    assert P.hamming_table(descs[2], descs[0])[0, 0] == tau and P.hamming_table(descs[3], descs[1])[0, 0] == tau + 1
    seqs, frames = [0, 1, 0, 1], [0, 0, 10, 10]
    db = vo.place_db(rows=40, capacity=4, with_geometry=False)
    try:
        ref = P.PlaceRef(40, 4)
        _add(vo, db, descs, seqs, frames); ref.add(descs, [copies] * 4, seqs, frames)
        want = ref.score(2, 2, tau, 10)
        assert want.tolist() == [[copies, -1, -1, -1], [-1, 0, -1, -1]]
        assert np.array_equal(_score(vo, db, 2, 2, tau, 10), want)
    finally:
        db.close()


def test_score_gap_boundary(vo, synth):
    """frame_c = frame_q - min_gap is eligible, frame_c = frame_q - min_gap + 1 is not"""
    rng = np.random.default_rng(4)
    frames = [0, 3, 4, 7, 8, 10]
    descs = _entries(synth, rng, [40] * 6)
    db = vo.place_db(rows=64, capacity=8, with_geometry=False)
    try:
        ref = P.PlaceRef(64, 8)
        _add(vo, db, descs, [0] * 6, frames); ref.add(descs, [40] * 6, [0] * 6, frames)
        got = _score(vo, db, 0, 6, 30, 3)
        assert np.array_equal(got, ref.score(0, 6, 30, 3))
        assert got[5, 3] >= 0 and got[5, 4] == -1 and got[3, 2] >= 0 and got[4, 3] == -1 and got[2, 0] >= 0 and got[1, 0] >= 0 and got[0, 0] == -1
    finally:
        db.close()


def test_score_more_rows_than_one_workgroup(vo, synth):
    """600 rows per entry: the query's rows span two column blocks whose counts meet in the table"""
    rng = np.random.default_rng(5)
    ns = [600, 513, 37, 600]
    descs = _entries(synth, rng, ns, n_base=300)
    db = vo.place_db(rows=600, capacity=4, with_geometry=False)
    try:
        ref = P.PlaceRef(600, 4)
        _add(vo, db, descs, [0] * 4, [0, 1, 2, 3]); ref.add(descs, ns, [0] * 4, [0, 1, 2, 3])
        want = ref.score(0, 4, 30, 1)
        assert np.array_equal(_score(vo, db, 0, 4, 30, 1), want) and want[3, 0] > 100
    finally:
        db.close()


def test_select(vo):
    """ties, the min_score boundary, K = 8 with three eligible entries, a query with none"""
    import torch
    score = np.array([[5, -1, 7, 5, 0, 7, 3, -77, -77],
                      [-1, -1, -1, -1, -1, -1, -1, -77, -77],
                      [0, 4, -1, 4, -1, -1, -1, -77, -77],
                      [9, 9, 9, 9, 9, 9, 9, -77, -77]], np.int32)   # ld = 9 above the seven entries
    db = vo.place_db(rows=8, capacity=7, with_geometry=False)
    try:
        _add(vo, db, [np.zeros((0, 32), np.uint8)] * 7, [0] * 7, list(range(7)))
        ds = torch.from_numpy(score).to(_dev())
        for K, min_score in ((3, 1), (8, 0), (2, -5), (4, 5), (4, 6), (1, 4), (8, 4)):
            dc, dcs = db.select(0, ds, K, min_score)
            vo.sync()
            wc, ws = P.select(score[:, :7], K, min_score)
            assert np.array_equal(dc.cpu().numpy(), wc) and np.array_equal(dcs.cpu().numpy(), ws), (K, min_score)
        assert P.select(score[:, :7], 8, 0)[0][2].tolist() == [1, 3, 0, -1, -1, -1, -1, -1]
    finally:
        db.close()


def test_add_masks_clamp_refusal_and_valid_rows(vo, pkg):
    rng = np.random.default_rng(6)
    R, kp_cap = 40, 50
    ns = [50, 12, 0, 33, 40]
    descs = [rng.integers(0, 256, (50, 32), dtype=np.uint8) for _ in ns]
    kps = [rng.uniform(0, 1000, (50, 2)).astype(np.float32) for _ in ns]
    xyz = [rng.normal(0, 10, (50, 3)).astype(np.float32) for _ in ns]
    valid = [(rng.random(50) < 0.6).astype(np.uint8) for _ in ns]
    seqs, frames, add = [3, 1, 4, 1, 5], [9, 2, 6, 5, 3], [1, 0, 1, 5, 1]
    db = vo.place_db(rows=R, capacity=5, with_geometry=True)
    try:
        ref = P.PlaceRef(R, 5)
        assert _add(vo, db, descs, seqs, frames, add=add, ns=ns, geom=(kps, xyz, valid), kp_cap=kp_cap) == 0
        assert ref.add(descs, ns, seqs, frames, add=add, valids=valid) == 0
        assert db.stats() == dict(n_entries=4, capacity=5, rows_per_entry=R, with_geometry=1, n_refused=0)

        def contents():
            out = []
            for e in range(len(db)):
                g = db.entry(e)
                out.append((g["n"], g["seq"], g["frame"], g["desc"].tobytes(), g["desc_tail"].tobytes(), g["xy"].tobytes(), g["xyz"].tobytes(), g["valid"].tobytes(),
                            g["qsel"].tobytes()))
            return out

        src = [b for b in range(5) if add[b]]
        for e, b in enumerate(src):
            g = db.entry(e); n = min(ns[b], R)
            assert (g["n"], g["seq"], g["frame"]) == (n, seqs[b], frames[b]) and np.array_equal(g["desc"], descs[b][:n]) and not g["desc_tail"].any()
            assert np.array_equal(g["xy"], kps[b][:n]) and np.array_equal(g["xyz"], xyz[b][:n]) and np.array_equal(g["valid"], valid[b][:n])
            assert np.array_equal(g["qsel"], np.flatnonzero(valid[b][:n])) and np.array_equal(g["qsel"], ref.qsel(e))
        before = contents()
        # two more do not fit one free slot: nothing is added, the refusal is counted
        with pytest.raises(pkg.VslamError, match="do not fit"):
            _add(vo, db, descs[:2], [0, 0], [0, 1], ns=[5, 5], geom=(kps[:2], xyz[:2], valid[:2]), kp_cap=kp_cap)
        assert db.stats()["n_entries"] == 4 and db.stats()["n_refused"] == 1 and contents() == before
        # a mask that adds nothing is no refusal; one entry still fits; rows at or past kp_capacity own no point
        assert _add(vo, db, descs[:2], [0, 0], [0, 1], add=[0, 0], geom=(kps[:2], xyz[:2], valid[:2]), kp_cap=kp_cap) == 4 and len(db) == 4
        assert _add(vo, db, descs[:1], [7], [8], geom=([kps[0]], [xyz[0]], [np.ones(50, np.uint8)]), kp_cap=30) == 4
        g = db.entry(4)
        assert g["n"] == 40 and np.array_equal(g["qsel"], np.arange(30)) and not g["valid"][30:].any() and contents()[:4] == before
        db.clear()
        assert db.stats()["n_entries"] == 0 and db.stats()["n_refused"] == 0
    finally:
        db.close()


def test_refused_arguments(vo, pkg):
    import torch
    lib = vo.lib
    no = _refusals(lib, pkg.VSLAM_ERR_ARG, "place")
    db = vo.place_db(rows=32, capacity=4, with_geometry=False)
    dbg = vo.place_db(rows=32, capacity=4, with_geometry=True)
    other = pkg.VO(device=0, max_batch=1)
    try:
        _add(vo, db, [np.zeros((3, 32), np.uint8)] * 3, [0] * 3, [0, 1, 2])
        buf = torch.zeros((4, 8), dtype=torch.int32, device=_dev()); T = torch.zeros((4, 7), dtype=torch.float64, device=_dev())
        desc = torch.zeros((2, 32, 32), dtype=torch.uint8, device=_dev()); ints = torch.zeros(8, dtype=torch.int32, device=_dev())
        torch.cuda.synchronize()
        p, d, n = buf.data_ptr(), desc.data_ptr(), ints.data_ptr()
        h = C.c_void_p()
        no("create null ctx", lib.vslam_place_create(None, 32, 4, 0, C.byref(h)))
        no("create rows 0", lib.vslam_place_create(vo.h, 0, 4, 0, C.byref(h)))
        no("create rows 4097", lib.vslam_place_create(vo.h, 4097, 4, 0, C.byref(h)))
        no("create capacity 0", lib.vslam_place_create(vo.h, 32, 0, 0, C.byref(h)))
        no("clear null database", lib.vslam_place_clear(None))
        no("stats null host", lib.vslam_place_stats(db.h, None))
        st = pkg.PlaceStats(); st.struct_size = 4
        no("stats struct_size", lib.vslam_place_stats(db.h, C.byref(st)))
        no("read_entry 3 of 3", lib.vslam_place_read_entry(db.h, 3, np.zeros(4, np.int32), None, None, None, None, None))
        add = lambda *a: lib.vslam_place_add_dev(*a)
        no("add a database of another context", add(other.h, db.h, d, 1024, n, None, n, n, None, None, None, 0, 2, None))
        no("add null database", add(vo.h, None, d, 1024, n, None, n, n, None, None, None, 0, 2, None))
        no("add null d_desc", add(vo.h, db.h, None, 1024, n, None, n, n, None, None, None, 0, 2, None))
        no("add null d_n", add(vo.h, db.h, d, 1024, None, None, n, n, None, None, None, 0, 2, None))
        no("add null d_seq", add(vo.h, db.h, d, 1024, n, None, None, n, None, None, None, 0, 2, None))
        no("add null d_frame", add(vo.h, db.h, d, 1024, n, None, n, None, None, None, None, 0, 2, None))
        no("add B 0", add(vo.h, db.h, d, 1024, n, None, n, n, None, None, None, 0, 0, None))
        no("add d_desc not aligned", add(vo.h, db.h, d + 4, 1024, n, None, n, n, None, None, None, 0, 2, None))
        no("add stride not aligned", add(vo.h, db.h, d, 1000, n, None, n, n, None, None, None, 0, 2, None))
        no("add geometry wanted, not given", add(vo.h, dbg.h, d, 1024, n, None, n, n, None, None, None, 32, 2, None))
        score = lambda *a: lib.vslam_place_score_dev(*a)
        no("score a database of another context", score(other.h, db.h, 0, 3, 30, 1, p, 8))
        no("score null d_score", score(vo.h, db.h, 0, 3, 30, 1, None, 8))
        no("score nq 0", score(vo.h, db.h, 0, 0, 30, 1, p, 8))
        no("score q0 -1", score(vo.h, db.h, -1, 2, 30, 1, p, 8))
        no("score range past the entries", score(vo.h, db.h, 2, 2, 30, 1, p, 8))
        no("score tau -1", score(vo.h, db.h, 0, 3, -1, 1, p, 8))
        no("score tau 256", score(vo.h, db.h, 0, 3, 256, 1, p, 8))
        no("score ld below n_entries", score(vo.h, db.h, 0, 3, 30, 1, p, 2))
        sel = lambda *a: lib.vslam_place_select_dev(*a)
        no("select a database of another context", sel(other.h, db.h, 0, 3, p, 8, 3, 1, p, p))
        no("select null d_score", sel(vo.h, db.h, 0, 3, None, 8, 3, 1, p, p))
        no("select null d_cand", sel(vo.h, db.h, 0, 3, p, 8, 3, 1, None, p))
        no("select null d_cand_score", sel(vo.h, db.h, 0, 3, p, 8, 3, 1, p, None))
        no("select K 0", sel(vo.h, db.h, 0, 3, p, 8, 0, 1, p, p))
        no("select K 9", sel(vo.h, db.h, 0, 3, p, 8, 9, 1, p, p))
        no("select ld below n_entries", sel(vo.h, db.h, 0, 3, p, 2, 3, 1, p, p))
        no("select range past the entries", sel(vo.h, db.h, 1, 3, p, 8, 3, 1, p, p))
        ver = lambda *a: lib.vslam_place_verify_dev(*a)
        t = T.data_ptr()
        no("verify no geometry", ver(vo.h, db.h, 0, 3, p, 3, 0, 10, t, n, n))
        _add(vo, dbg, [np.zeros((3, 32), np.uint8)] * 3, [0] * 3, [0, 1, 2], geom=([np.zeros((3, 2), np.float32)] * 3, [np.zeros((3, 3), np.float32)] * 3, [np.ones(3, np.uint8)] * 3))
        no("verify a database of another context", ver(other.h, dbg.h, 0, 1, p, 3, 0, 10, t, n, n))
        no("verify null d_cand", ver(vo.h, dbg.h, 0, 3, None, 3, 0, 10, t, n, n))
        no("verify null d_T_q_c", ver(vo.h, dbg.h, 0, 3, p, 3, 0, 10, None, n, n))
        no("verify null d_n_matches", ver(vo.h, dbg.h, 0, 3, p, 3, 0, 10, t, None, n))
        no("verify null d_n_inliers", ver(vo.h, dbg.h, 0, 3, p, 3, 0, 10, t, n, None))
        no("verify rank outside [0, K)", ver(vo.h, dbg.h, 0, 3, p, 3, 3, 10, t, n, n))
        no("verify K 9", ver(vo.h, dbg.h, 0, 3, p, 9, 0, 10, t, n, n))
        no("verify min_inliers -1", ver(vo.h, dbg.h, 0, 3, p, 3, 0, -1, t, n, n))
        no("verify range past the entries", ver(vo.h, dbg.h, 1, 3, p, 3, 0, 10, t, n, n))
        no("verify nq above max_batch", ver(vo.h, dbg.h, 0, vo.params.max_batch + 1, p, 3, 0, 10, t, n, n))
        assert db.stats()["n_entries"] == 3 and db.stats()["n_refused"] == 0
    finally:
        other.close(); db.close(); dbg.close()


def _verify_case(synth, seed, M=120, n_out=25, n_extra=30):
    """the candidate entry holds M points (a fifth of them without a valid depth) and random descriptors; the query entry holds their projections
    under a known pose in shuffled order, descriptors a few bits away, n_out of them at wrong pixels, plus n_extra unrelated rows"""
    rng = np.random.default_rng(seed)
    p = synth.pnp_problem(M=M, seed=seed, outlier_frac=0.0)
    desc_c = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    valid_c = (rng.random(M) < 0.8).astype(np.uint8)
    perm = rng.permutation(M + n_extra)
    desc_q = rng.integers(0, 256, (M + n_extra, 32), dtype=np.uint8); uv_q = rng.uniform(0, 1200, (M + n_extra, 2)).astype(np.float32)
    d = desc_c.copy()
    for k in range(M):
        for _ in range(int(rng.integers(0, 9))):
            d[k, int(rng.integers(32))] ^= np.uint8(1 << int(rng.integers(8)))
    uv = p["uv"].copy()
    uv[rng.permutation(M)[:n_out]] += rng.uniform(-60, 60, (n_out, 2)).astype(np.float32)
    desc_q[perm[:M]] = d; uv_q[perm[:M]] = uv
    return dict(desc_c=desc_c, xyz_c=p["xyz"], valid_c=valid_c, desc_q=desc_q, uv_q=uv_q, T_true=p["T_true"])


def test_verify_against_the_entries_by_hand_and_the_oracle(vo, pkg, oracle, synth):
    import torch
    R = 160
    cases = [_verify_case(synth, s) for s in (3, 8)]
    db = vo.place_db(rows=R, capacity=8, with_geometry=True)
    try:
        z2 = lambda n: np.zeros((n, 2), np.float32)
        # entries 0, 1: the candidates (points, no pixels needed); entry 2: an unrelated place; entries 3, 4: the queries (pixels, no points); 5: no candidate
        descs = [cases[0]["desc_c"], cases[1]["desc_c"], np.random.default_rng(1).integers(0, 256, (90, 32), dtype=np.uint8), cases[0]["desc_q"], cases[1]["desc_q"],
                 cases[0]["desc_q"][:7]]
        kps = [z2(120), z2(120), z2(90), cases[0]["uv_q"], cases[1]["uv_q"], cases[0]["uv_q"][:7]]
        xyz = [cases[0]["xyz_c"], cases[1]["xyz_c"]] + [np.zeros((len(d), 3), np.float32) for d in descs[2:]]
        valid = [cases[0]["valid_c"], cases[1]["valid_c"]] + [np.zeros(len(d), np.uint8) for d in descs[2:]]
        _add(vo, db, descs, [0] * 6, [0, 1, 2, 20, 21, 22], geom=(kps, xyz, valid))
        cand = np.array([[0, 2, -1], [1, -1, -1], [-1, -1, -1]], np.int32)
        d_cand = torch.from_numpy(cand).to(_dev())
        got = {}
        for rank in (0, 1, 2):
            dT, dnm, dni = db.verify(3, d_cand, rank, min_inliers=10)
            vo.sync()
            got[rank] = (dT.cpu().numpy(), dnm.cpu().numpy(), dni.cpu().numpy())
        ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
        # the three existing entries by hand on buffers of the same content, the gather in numpy
        D = np.zeros((6, R, 32), np.uint8); n = np.zeros(6, np.int32); S = np.zeros((6, R), np.int32); ns = np.zeros(6, np.int32)
        for e in range(6):
            D[e, :len(descs[e])] = descs[e]; n[e] = len(descs[e])
            s = np.flatnonzero(valid[e]); S[e, :len(s)] = s; ns[e] = len(s)
        t = lambda a: torch.from_numpy(a).to(_dev())
        dD, dn, dS, dns = t(D), t(n), t(S), t(ns)
        for rank in (0, 1):
            qitem = t(cand[:, rank].copy()); gap = torch.ones(3, dtype=torch.float64, device=_dev())
            dm = torch.zeros((3, R, 16), dtype=torch.uint8, device=_dev()); dnm = torch.zeros(3, dtype=torch.int32, device=_dev())
            torch.cuda.synchronize()
            vo.feature_matching_pairs_dev(dD.data_ptr(), R * 32, dn.data_ptr(), dS.data_ptr(), dns.data_ptr(), R, qitem.data_ptr(), 6, dD[3:].data_ptr(), R * 32,
                                          dn[3:].data_ptr(), gap.data_ptr(), 1, 3, R, dm.data_ptr(), R, dnm.data_ptr())
            vo.sync()
            nm = dnm.cpu().numpy(); m = dm.cpu().numpy()
            X = np.zeros((3, R, 3), np.float32); U = np.zeros((3, R, 2), np.float32); npts = np.zeros(3, np.int32)
            for b in range(3):
                c = cand[b, rank]
                if c < 0 or nm[b] < 10:
                    continue
                mm = m[b].reshape(-1).view(pkg.DMATCH_DTYPE)[:nm[b]]
                X[b, :nm[b]] = xyz[c][mm["queryIdx"]]; U[b, :nm[b]] = kps[3 + b][mm["trainIdx"]]; npts[b] = nm[b]
            dX, dU, dnp = t(X), t(U), t(npts)
            dT = torch.zeros((3, 7), dtype=torch.float64, device=_dev()); dni = torch.zeros(3, dtype=torch.int32, device=_dev())
            torch.cuda.synchronize()
            vo.pnp_ransac_dev(dX.data_ptr(), dU.data_ptr(), dnp.data_ptr(), R, 3, dT.data_ptr(), 100, vo.params.pnp_reproj_thr, 0.99, None, dni.data_ptr(), None)
            vo.sync()
            gT, gnm, gni = got[rank]
            assert gT.tobytes() == dT.cpu().numpy().tobytes() and np.array_equal(gni, dni.cpu().numpy()), rank
            assert np.array_equal(gnm, np.where(cand[:, rank] >= 0, nm, 0))
            # ... and the oracle's matcher + RANSAC
            for b in range(3):
                c = cand[b, rank]
                if c < 0:
                    assert gnm[b] == 0 and gni[b] == 0 and np.array_equal(gT[b], ident)
                    continue
                sel = np.flatnonzero(valid[c])
                om = oracle.feature_matching(np.ascontiguousarray(descs[c][sel]), descs[3 + b], 1.0)
                assert gnm[b] == len(om), (rank, b)
                if len(om) < 10:
                    assert gni[b] == 0 and np.array_equal(gT[b], ident)
                    continue
                wT, winl, wn, wit = oracle.pnp_ransac(xyz[c][sel[om["queryIdx"]]], kps[3 + b][om["trainIdx"]])
                assert gni[b] == wn, (rank, b, gni[b], wn)
                assert np.allclose(gT[b], wT, rtol=1e-4, atol=1e-6), (rank, b)
        gT, gnm, gni = got[0]
        assert gni[0] >= 50 and gni[1] >= 50 and gnm[0] > gni[0]                       # the true candidates: most valid points, minus the planted outliers
        for b in (0, 1):                                                                # (q and -q are one rotation)
            assert np.allclose(gT[b][4:], cases[b]["T_true"][4:], atol=0.1) and abs(np.dot(gT[b][:4], cases[b]["T_true"][:4])) > 0.9999
        assert got[1][1][0] == 0 and got[1][2][0] == 0                                  # the unrelated place has no valid point: no match, no edge
        assert (got[2][1] == 0).all() and (got[2][2] == 0).all() and all(np.array_equal(got[2][0][b], ident) for b in range(3))
    finally:
        db.close()
