"""CPU: known answers for the numpy restatement of the rectification arithmetic itself (tests/rectify_ref.py), so that the yardstick of
tests/test_rectify_params.py and tests/test_gpu_rectify.py is not merely self-consistent."""
import numpy as np

import rectify_ref as RR


def _img(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def test_identity_map_returns_the_image():
    c = RR.cam((300.0, 310.0, 150.5, 99.25))
    xy, frac = RR.build_maps(c, 64, 40)
    x, y = np.meshgrid(np.arange(64), np.arange(40))
    assert np.array_equal(xy[..., 0], x) and np.array_equal(xy[..., 1], y) and not frac.any()
    img = _img(40, 64)
    assert np.array_equal(RR.remap(img, xy, frac), img)


def test_principal_point_shift_moves_the_image_by_whole_columns():
    """cx' = cx + 3: destination column x shows source column x - 3, and the first three columns lie outside the source (0)"""
    K = (300.0, 310.0, 150.5, 99.25)
    c = RR.cam(K, P=(K[0], K[1], K[2] + 3, K[3]))
    xy, frac = RR.build_maps(c, 64, 40)
    img = _img(40, 64, 1)
    out = RR.remap(img, xy, frac)
    assert not frac.any()
    assert np.array_equal(out[:, 3:], img[:, :-3]) and not out[:, :3].any()


def test_half_pixel_shift_is_the_rounded_mean():
    """cx' = cx - 0.5: u = x + 0.5, ax = 16, so dst = (16 * 32 * a + 16 * 32 * b + 512) >> 10 = (a + b + 1) >> 1 exactly"""
    K = (256.0, 256.0, 32.0, 20.0)   # (powers of two: x + 0.5 is exact in double, no tie is decided by a rounding error)
    c = RR.cam(K, P=(K[0], K[1], K[2] - 0.5, K[3]))
    xy, frac = RR.build_maps(c, 64, 40)
    assert (frac == 16).all() and np.array_equal(xy[..., 0], np.broadcast_to(np.arange(64), (40, 64)))
    img = _img(40, 64, 2)
    out = RR.remap(img, xy, frac)
    a = img[:, :-1].astype(np.int32); b = img[:, 1:].astype(np.int32)
    assert np.array_equal(out[:, :-1], (a + b + 1) >> 1)
    assert np.array_equal(out[:, -1], (img[:, -1].astype(np.int32) + 0 + 1) >> 1)   # the right tap of the last column is outside: 0, per tap


def test_taps_outside_count_as_zero_per_tap():
    """by hand on a 3 x 3 image: every entry has some taps inside and some outside"""
    src = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    xy = np.array([[[-1, -1], [2, 2], [-1, 1]], [[2, 0], [1, -1], [-2, 0]]], np.int16)
    ax = np.array([[16, 8, 31], [4, 0, 16]]); ay = np.array([[16, 24, 0], [0, 16, 16]])
    frac = (ay * 32 + ax).astype(np.uint16)
    want = np.array([
        [(16 * 16 * 10 + 512) >> 10,                 # only the lower right tap (0, 0) is inside
         (24 * 8 * 90 + 512) >> 10,                  # only the upper left tap (2, 2)
         (31 * 32 * 40 + 512) >> 10],                # taps (-1, 1) outside, (0, 1) = 40 with ax (32 - ay); the lower row has weight 0
        [(28 * 32 * 30 + 512) >> 10,                 # (2, 0) = 30 with (32 - 4) * 32; (3, 0) outside
         (32 * 16 * 20 + 512) >> 10,                 # row -1 outside; (1, 0) = 20 with (32 - 0) * 16
         0],                                         # columns -2 and -1: everything outside
    ], np.uint8)
    assert np.array_equal(RR.remap(src, xy, frac), want)


def test_nonfinite_coordinates_become_outside_entries():
    """W = 0 on a destination line: the entries there are (-32768, -32768, 0) and read 0"""
    c = RR.cam((100.0, 100.0, 8.0, 8.0), R=RR._rot_xyz(0, 90.0, 0), P=(100.0, 100.0, 8.0, 8.0))
    u32, _ = RR.coords32(c, 17, 9)
    xy, frac = RR.build_maps(c, 17, 9)
    bad = ~np.isfinite(u32)
    assert (xy[bad] == -32768).all() and not frac[bad].any()
    assert np.abs(xy.astype(np.int64)).max() <= 32768


def test_strong_rig_leaves_the_source_at_the_corners():
    """the 5 degree roll (left: +5, right: -5) turns two opposite destination corners of each camera out of the source, all four between the two"""
    r = RR.RIGS["strong"]
    sw, sh = r["src"]
    outside = []
    for c in r["cams"]:
        xy, _ = RR.build_maps(c, *r["dst"])
        sx, sy = xy[..., 0].astype(int), xy[..., 1].astype(int)
        o = (sx < -1) | (sx >= sw) | (sy < -1) | (sy >= sh)   # all four taps outside
        assert 0.02 < o.mean() < 0.1
        outside.append([bool(o[y, x]) for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1))])
        assert any(c["D"][5:] != 0)
    assert outside[0] == [False, True, True, False] and outside[1] == [True, False, False, True]
