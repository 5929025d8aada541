"""GPU: vslam_feature_matching_subset_dev -- the batched matcher on an ascending subset of every item's query rows -- against the oracle's matcher
on the gathered rows (integers and distances exactly equal), the unmasked entry bit for bit on the full selection, and the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(vo, pkg, qs, ts, sels, cap, gate=1, out_cap=None, subset=True, sel_cap=None):
    """one batched call on items (q rows, t rows, ascending selection); returns [(DMATCH array)] per item and the raw output bytes"""
    import torch
    B = len(qs)
    out_cap = cap if out_cap is None else out_cap
    sel_cap = cap if sel_cap is None else sel_cap
    dev = torch.device("cuda:0")
    Q = np.zeros((B, cap, 32), np.uint8); T = np.zeros((B, cap, 32), np.uint8); S = np.full((B, sel_cap), -1, np.int32)
    for b in range(B):
        Q[b, :len(qs[b])] = qs[b]; T[b, :len(ts[b])] = ts[b]; S[b, :len(sels[b])] = sels[b]
    dq, dt, ds = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(S).to(dev)
    dnq = torch.tensor([len(q) for q in qs], dtype=torch.int32, device=dev); dnt = torch.tensor([len(t) for t in ts], dtype=torch.int32, device=dev)
    dns = torch.tensor([len(s) for s in sels], dtype=torch.int32, device=dev)
    dgap = torch.ones(B, dtype=torch.float64, device=dev)
    dout = torch.zeros((B, out_cap, 16), dtype=torch.uint8, device=dev); dn = torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if subset:
        vo.feature_matching_subset_dev(dq.data_ptr(), cap * 32, dnq.data_ptr(), ds.data_ptr(), dns.data_ptr(), sel_cap, dt.data_ptr(), cap * 32,
                                       dnt.data_ptr(), dgap.data_ptr(), gate, B, cap, dout.data_ptr(), out_cap, dn.data_ptr())
    else:
        vo.feature_matching_dev(dq.data_ptr(), cap * 32, dnq.data_ptr(), dt.data_ptr(), cap * 32, dnt.data_ptr(), dgap.data_ptr(), gate, B, cap,
                                dout.data_ptr(), out_cap, dn.data_ptr())
    vo.sync()
    out, n = dout.cpu().numpy(), dn.cpu().numpy()
    got = [out[b].reshape(-1).view(pkg.DMATCH_DTYPE)[:n[b]].copy() for b in range(B)]
    # only the first n entries of an item are defined output
    raw = b"".join(got[b].tobytes() for b in range(B)) + n.tobytes()
    return got, raw


def _expect(oracle, q, t, sel, gate=1):
    sel = np.asarray(sel, np.int64)
    if len(sel) == 0 or len(t) == 0:
        return np.zeros(0, oracle.DMATCH_DTYPE)
    g = np.ascontiguousarray(q[sel])
    m = oracle.feature_matching(g, t, 1.0) if gate else oracle.bf_match_xcheck(g, t)
    m = m.copy()
    m["queryIdx"] = sel[m["queryIdx"]]
    return m


def _same(got, want, tag=None):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in ("queryIdx", "trainIdx", "distance"):
        assert np.array_equal(got[f], want[f]), (tag, f)


def _items(synth, rng, shapes):
    """[(q, t)] with near-duplicate query rows planted (ties and near-ties: which rows are selected decides who wins the cross-check)"""
    qs, ts = [], []
    for k, (n1, n2) in enumerate(shapes):
        q, t = synth.random_descriptors(n1, n2, seed=int(rng.integers(1 << 30)))
        q = q.copy()
        if n1 >= 4:
            src = rng.permutation(n1)[:n1 // 4]; dst = rng.permutation(n1)[:len(src)]
            q[dst] = q[src]                       # exact duplicates: first-minimum ties in the row order
            for d in dst[::2]:
                q[d, int(rng.integers(32))] ^= np.uint8(1 << int(rng.integers(8)))
        qs.append(q); ts.append(t)
    return qs, ts


@pytest.mark.parametrize("gate", [1, 0])
def test_subset_against_the_oracle_on_gathered_rows(vo, pkg, oracle, synth, gate):
    """one batch of four items with different nq, nt and selection sizes -- a random third of 1500 rows, one row, a count that is no multiple of 32,
    an empty selection -- and a second of random selections of 1500-row items; a 4-item batch of capacity 1536 takes the query-split path"""
    rng = np.random.default_rng(71 + gate)
    cap = 1536
    qs, ts = _items(synth, rng, [(1500, 1500), (900, 1300), (1237, 777), (640, 1500)])
    sels = [np.sort(rng.permutation(1500)[:500]), np.array([417]), np.sort(rng.permutation(1237)[:333]), np.zeros(0, np.int64)]
    got, raw = _run(vo, pkg, qs, ts, sels, cap, gate)
    for b in range(4):
        _same(got[b], _expect(oracle, qs[b], ts[b], sels[b], gate), (gate, b))
    assert len(got[3]) == 0 and len(got[1]) <= 1
    assert raw == _run(vo, pkg, qs, ts, sels, cap, gate)[1], "run twice: identical bytes"
    qs, ts = _items(synth, rng, [(1500, 1500)] * 4)
    sels = [np.sort(rng.permutation(1500)[:n]) for n in (1499, 750, 97, 31)]
    got, _ = _run(vo, pkg, qs, ts, sels, cap, gate)
    for b in range(4):
        _same(got[b], _expect(oracle, qs[b], ts[b], sels[b], gate), (gate, "1500", b))


@pytest.mark.parametrize("gate", [1, 0])
def test_full_selection_is_the_unmasked_entry_bit_for_bit(vo, pkg, oracle, synth, gate):
    rng = np.random.default_rng(75)
    cap = 1536
    qs, ts = _items(synth, rng, [(1500, 1500), (1001, 1300), (33, 64), (1, 5)])
    sels = [np.arange(len(q)) for q in qs]
    a, ra = _run(vo, pkg, qs, ts, sels, cap, gate)
    b, rb = _run(vo, pkg, qs, ts, sels, cap, gate, subset=False)
    assert ra == rb
    for k in range(4):
        _same(a[k], _expect(oracle, qs[k], ts[k], sels[k], gate), k)


def test_out_capacity_cut(vo, pkg, oracle, synth):
    rng = np.random.default_rng(76)
    qs, ts = _items(synth, rng, [(1200, 1200), (800, 900)])
    sels = [np.sort(rng.permutation(1200)[:700]), np.sort(rng.permutation(800)[:400])]
    got, _ = _run(vo, pkg, qs, ts, sels, 1536, 0, out_cap=100)
    for b in range(2):
        want = _expect(oracle, qs[b], ts[b], sels[b], 0)
        assert len(want) > 100
        _same(got[b], want[:100], b)


def test_large_batch_without_query_split(pkg, oracle, synth):
    """512 items of capacity 1024 fill the chip without splitting the query range (launch_match: 2 column blocks x 512 items): the plain-store path of
    the train-nearest kernel, items of different nq, nt and selection sizes, against the oracle and against the unmasked entry on the full selection"""
    rng = np.random.default_rng(77)
    B, cap = 512, 1024
    vo = pkg.VO(params=pkg.default_params(max_batch=B), device=0)
    try:
        shapes = [(int(rng.integers(40, 260)), int(rng.integers(40, 260))) for _ in range(B)]
        shapes[0] = (1024, 1024); shapes[1] = (1000, 600)
        qs, ts = _items(synth, rng, shapes)
        sels = [np.sort(rng.permutation(n1)[:int(rng.integers(0, n1 + 1))]) for n1, _ in shapes]
        sels[0] = np.sort(rng.permutation(1024)[:345])
        got, raw = _run(vo, pkg, qs, ts, sels, cap, 1)
        for b in range(B):
            _same(got[b], _expect(oracle, qs[b], ts[b], sels[b], 1), b)
        assert raw == _run(vo, pkg, qs, ts, sels, cap, 1)[1]
        full = [np.arange(n1) for n1, _ in shapes]
        assert _run(vo, pkg, qs, ts, full, cap, 1)[1] == _run(vo, pkg, qs, ts, full, cap, 1, subset=False)[1]
    finally:
        vo.close()


def test_refusals(vo, pkg):
    import torch
    dev = torch.device("cuda:0")
    cap = 64
    d = torch.zeros((1, cap, 32), dtype=torch.uint8, device=dev); n = torch.full((1,), 8, dtype=torch.int32, device=dev)
    sel = torch.arange(cap, dtype=torch.int32, device=dev); gap = torch.ones(1, dtype=torch.float64, device=dev)
    out = torch.zeros((1, cap, 16), dtype=torch.uint8, device=dev); no = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(qsel=sel.data_ptr(), nqsel=n.data_ptr(), sel_cap=cap, dq=d.data_ptr(), stride=cap * 32, out_cap=cap):
        vo.feature_matching_subset_dev(dq, stride, n.data_ptr(), qsel, nqsel, sel_cap, d.data_ptr(), cap * 32, n.data_ptr(), gap.data_ptr(), 1, 1, cap,
                                       out.data_ptr(), out_cap, no.data_ptr())
    call(); vo.sync()
    for kw in (dict(qsel=None), dict(nqsel=None), dict(sel_cap=0), dict(sel_cap=4097), dict(dq=d.data_ptr() + 8), dict(stride=cap * 32 + 8), dict(out_cap=0)):
        with pytest.raises(pkg.VslamError):
            call(**kw)
