"""GPU: the batched geometry entries (vslam_triangulate_dev, vslam_find_3d_disparity_dev) on ragged items: B = 5, capacity 300,
d_n = [0, 1, 256, 257, 400] (empty, one row, one full block, one row into the second block, a count above the capacity), every item with its own
pose (a real rotation) and, for find_3d, its own 64 x 48 disparity map.  Two yardsticks per item: the host-tier call of the same library on the item
alone (byte for byte: it runs the same launch at B = 1) and the CPU oracle at the tolerances of tests/test_gpu_geom.py (flags equal, rtol 1e-4 /
atol 1e-5 on the valid points).  Rows at or past min(d_n[b], capacity) must keep the poison the buffers were filled with.

Each non-empty item starts with the gate edges the f32 inputs can hit exactly:
  find_3d      for each of depth_min, depth_max, depth_reliable the two ADJACENT f32 disparities between which fx * b / d crosses the gate (found on
               the CPU; the oracle's own flags must differ across each pair -- all three pairs separate: one f32 step of d moves the f64 depth by
               1e-7 relative, nine orders above an f64 step, so none had to be dropped);
  triangulate  uL == uR, uL < uR (both fail the positive-disparity gate), |vL - vR| exactly row_tol (passes) and the next f32 above it (fails), in
               both directions.
The one-row item carries one edge row per entry."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, CAP = 5, 300
NS = np.array([0, 1, 256, 257, 400], np.int32)
H, W = 48, 64
P_XYZ, P_FLAG = np.float32(-777.25), 0xEE


def _cam(vo):
    p = vo.params
    return np.array(list(p.cam)), (p.depth_min, p.depth_max, p.depth_reliable), p.stereo_row_tol


def _poses(synth):
    rng = np.random.default_rng(11)
    return np.stack([synth.perturb_pose(synth.se3_from_Rt(np.eye(3), [0.3 * b, -0.1, 2.0 - b]), rng, 0.3) for b in range(B)])


def _cuda(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def _outputs():
    import torch
    return (torch.full((B, CAP, 3), float(P_XYZ), dtype=torch.float32, device="cuda"), torch.full((B, CAP), P_FLAG, dtype=torch.uint8, device="cuda"),
            torch.full((B, CAP), P_FLAG, dtype=torch.uint8, device="cuda"))


def _check(got, b, n, host, want):
    """item b's first n rows against the host tier (bytes) and the oracle; the rows past n against the poison"""
    gx, gv, gr = (g[b] for g in got)
    for g, h_ in zip((gx[:n], gv[:n], gr[:n]), host):
        assert g.tobytes() == h_.tobytes(), b
    wx, wv, wr = want
    assert np.array_equal(gv[:n], wv) and np.array_equal(gr[:n], wr), b
    ok = wv.astype(bool)
    assert np.allclose(gx[:n][ok], wx[ok], rtol=1e-4, atol=1e-5), b
    assert (gx[n:] == P_XYZ).all() and (gv[n:] == P_FLAG).all() and (gr[n:] == P_FLAG).all(), b


def _crossing(fxb, gate):
    """the adjacent f32 disparities (lo, hi) with fx b / lo > gate >= fx b / hi, the arithmetic of both implementations (f64 division of the f32)"""
    d = np.float32(fxb / gate)
    while fxb / float(d) <= gate:
        d = np.nextafter(d, np.float32(0))
    while fxb / float(np.nextafter(d, np.float32(np.inf))) > gate:
        d = np.nextafter(d, np.float32(np.inf))
    return d, np.nextafter(d, np.float32(np.inf))


def test_find_3d_disparity_dev_ragged(vo, oracle, synth):
    cam, gate, _ = _cam(vo)
    T = _poses(synth)
    rng = np.random.default_rng(12)
    disp = rng.uniform(0.5, 90, (B, H, W)).astype(np.float32)
    disp[rng.random((B, H, W)) < 0.1] = -1.0
    disp[rng.random((B, H, W)) < 0.02] = 0.0
    kps = np.zeros((B, CAP), oracle.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(-2, W + 2, (B, CAP)).astype(np.float32); kps["y"] = rng.uniform(-2, H + 2, (B, CAP)).astype(np.float32)   # some fall outside the map
    edges = [d for g in gate for d in _crossing(cam[0] * cam[4], g)]      # (min lo, min hi, max lo, max hi, reliable lo, reliable hi)
    for b in range(B):
        for k, d in enumerate(edges):                                     # item b keeps its edge disparities in row b + 1 of ITS map
            disp[b, b + 1, 2 * k + 1] = d
            kps["x"][b, k] = 2 * k + 1 + 0.2 * b; kps["y"][b, k] = b + 1 + 0.5     # fractional pixels: the lookup truncates
    kps["x"][1, 0] = kps["x"][1, 1]; kps["y"][1, 0] = kps["y"][1, 1]      # the one-row item: the far side of depth_min
    # the oracle separates every pair
    wx, wv, wr = oracle.find_3d_disparity(kps[4, :6], disp[4], T[4], cam, gate)
    assert wv.tolist() == [1, 0, 0, 1, 1, 1] and wr.tolist() == [1, 0, 0, 0, 0, 1]
    import torch
    dK, dn, dD, dT = _cuda(kps), _cuda(NS), _cuda(disp), _cuda(T)
    out = _outputs()
    torch.cuda.synchronize()
    vo.find_3d_disparity_dev(dK.data_ptr(), dn.data_ptr(), CAP, B, dD.data_ptr(), W, H, dT.data_ptr(), *(o.data_ptr() for o in out))
    vo.sync()
    got = [o.cpu().numpy() for o in out]
    seen = np.zeros(2, int)
    for b in range(B):
        n = min(int(NS[b]), CAP)
        want = oracle.find_3d_disparity(kps[b, :n], disp[b], T[b], cam, gate)
        _check(got, b, n, vo.find_3d_disparity(kps[b, :n], disp[b], T[b]), want)
        seen += (int(want[1].sum()), n - int(want[1].sum()))
    assert got[1][1, 0] == 0                                              # (the one row: just past depth_min)
    assert seen.min() > 100
    # item b read pose b and map b: the neighbour's would not do
    other = oracle.find_3d_disparity(kps[3, :257], disp[2], T[3], cam, gate)
    assert not np.array_equal(other[1], got[1][3, :257])
    other = oracle.find_3d_disparity(kps[3, :257], disp[3], T[2], cam, gate)
    assert not np.allclose(other[0], got[0][3, :257], rtol=1e-4, atol=1e-5)


def test_triangulate_dev_ragged(vo, oracle, synth):
    cam, gate, row_tol = _cam(vo)
    assert row_tol == 2.0
    T = _poses(synth)
    rng = np.random.default_rng(13)
    Z = rng.uniform(2, 600, (B, CAP))
    uL = rng.uniform(0, 1241, (B, CAP)); v = rng.uniform(0, 376, (B, CAP))
    L = np.stack([uL, v], -1).astype(np.float32)
    R = np.stack([uL - cam[0] * cam[4] / Z + rng.normal(0, 0.3, (B, CAP)), v + rng.normal(0, 0.9, (B, CAP))], -1).astype(np.float32)
    up = np.nextafter(np.float32(row_tol), np.float32(np.inf))            # the next f32 above row_tol
    # (uL, vL, uR, vR); a disparity of 30 px is a depth of 13.7 m: inside every gate, so the row gate alone decides rows 2..5
    edge = [(700.0, 100.0, 700.0, 100.0), (700.0, 100.0, 700.5, 100.0),
            (700.0, row_tol, 670.0, 0.0), (700.0, up, 670.0, 0.0), (700.0, 0.0, 670.0, row_tol), (700.0, 0.0, 670.0, up)]
    for b in range(B):
        for k, e in enumerate(edge):
            L[b, k] = (e[0] + b, e[1]); R[b, k] = (e[2] + b, e[3])
    L[1, 0], R[1, 0] = L[1, 3], R[1, 3]                                   # the one-row item: one f32 step past row_tol
    wx, wv, wr = oracle.triangulate_dlt(L[4, :6], R[4, :6], T[4], cam, row_tol, gate)
    assert wv.tolist() == [0, 0, 1, 0, 1, 0] and wr.tolist() == wv.tolist()
    import torch
    dL, dR, dn, dT = _cuda(L), _cuda(R), _cuda(NS), _cuda(T)
    out = _outputs()
    torch.cuda.synchronize()
    vo.triangulate_dev(dL.data_ptr(), dR.data_ptr(), dn.data_ptr(), CAP, B, dT.data_ptr(), *(o.data_ptr() for o in out))
    vo.sync()
    got = [o.cpu().numpy() for o in out]
    seen = np.zeros(2, int)
    for b in range(B):
        n = min(int(NS[b]), CAP)
        want = oracle.triangulate_dlt(L[b, :n], R[b, :n], T[b], cam, row_tol, gate)
        _check(got, b, n, vo.triangulate(L[b, :n], R[b, :n], T[b]), want)
        seen += (int(want[1].sum()), n - int(want[1].sum()))
    assert got[1][1, 0] == 0
    assert seen.min() > 100
    other = oracle.triangulate_dlt(L[3, :257], R[3, :257], T[2], cam, row_tol, gate)   # item 3 under item 2's pose
    assert not np.allclose(other[0], got[0][3, :257], rtol=1e-4, atol=1e-5)
