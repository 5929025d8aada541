"""CPU (no GPU): the host-only half of the rectification stage through libvslam_hip.so -- vslam_rectify_params_check names every refused field,
and vslam_rectify_build_maps equals the numpy restatement tests/rectify_ref.py on every rig and camera."""
import ctypes as C
import math

import numpy as np
import pytest

import rectify_ref as RR


def _refused(pkg, p, w, h, *names):
    with pytest.raises(pkg.VslamError) as e:
        pkg.rectify_params_check(p, w, h)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_default_params_are_the_identity_rig(pkg):
    p = pkg.default_rectify_params()
    assert (p.src_w, p.src_h, p.struct_size) == (1241, 376, C.sizeof(pkg.RectifyParams)) and C.sizeof(pkg.RectifyParams) == 8 + 2 * 25 * 8 + 8
    for c in p.cam:
        assert list(c.K) == list(c.P) == [718.856, 718.856, 607.1928, 185.2157] and not any(c.D) and list(c.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert pkg.rectify_params_check(p, 1241, 376)
    x, y = np.meshgrid(np.arange(1241), np.arange(376))
    for cam in (0, 1):
        xy, frac = pkg.rectify_build_maps(p, cam, 1241, 376)
        assert xy.dtype == np.int16 and frac.dtype == np.uint16
        assert np.array_equal(xy[..., 0], x) and np.array_equal(xy[..., 1], y) and not frac.any()


@pytest.mark.parametrize("rig", sorted(RR.RIGS))
def test_accepted_rigs_pass(pkg, rig):
    assert pkg.rectify_params_check(RR.params_of(pkg, rig), *RR.RIGS[rig]["dst"])


def test_every_refused_field_is_named(pkg):
    mk = lambda: RR.params_of(pkg, "kitti_raw_like")
    w, h = RR.RIGS["kitti_raw_like"]["dst"]
    p = mk(); p.struct_size -= 8
    _refused(pkg, p, w, h, "struct_size")
    for field in ("src_w", "src_h"):
        for v in (1, 0, -5, 4097):
            p = mk(); setattr(p, field, v)
            _refused(pkg, p, w, h, field, str(v))
        for v in (2, 4096):
            p = mk(); setattr(p, field, v)
            assert pkg.rectify_params_check(p, w, h)
    for v in (1, 4097, -1):
        _refused(pkg, mk(), v, h, "dst_w", str(v))
        _refused(pkg, mk(), w, v, "dst_h", str(v))
    assert pkg.rectify_params_check(mk(), 2, 4096)
    for s in (0, 1):
        for name, n in (("K", 4), ("D", 8), ("R", 9), ("P", 4)):
            for i in range(n):
                for bad in (math.nan, math.inf, -math.inf):
                    p = mk(); getattr(p.cam[s], name)[i] = bad
                    _refused(pkg, p, w, h, "cam[%d].%s[%d]" % (s, name, i), "finite")
        for name in ("K", "P"):
            for i in (0, 1):
                for bad in (0.0, -700.0):
                    p = mk(); getattr(p.cam[s], name)[i] = bad
                    _refused(pkg, p, w, h, "cam[%d].%s[%d]" % (s, name, i))
        p = mk(); p.cam[s].R[0] *= 1 + 1e-5                 # not orthonormal
        _refused(pkg, p, w, h, "cam[%d].R" % s, "rotation")
        p = mk(); p.cam[s].R[4] += 3e-6
        _refused(pkg, p, w, h, "cam[%d].R" % s)
        p = mk()                                            # a reflection: orthonormal, det = -1
        for i in range(3):
            p.cam[s].R[i] = -p.cam[s].R[i]
        _refused(pkg, p, w, h, "cam[%d].R" % s, "det")
        p = mk(); p.cam[s].R[0] *= 1 + 1e-8                 # within the 1e-6 bound: accepted
        assert pkg.rectify_params_check(p, w, h)
    lib = pkg.load_library()
    assert lib.vslam_rectify_params_check(None, w, h) == pkg.VSLAM_ERR_ARG
    # build_maps runs the check first and refuses a bad camera index / null output
    p = mk(); p.src_w = 1
    with pytest.raises(pkg.VslamError):
        pkg.rectify_build_maps(p, 0, w, h)
    xy = np.zeros((h, w, 2), np.int16); fr = np.zeros((h, w), np.uint16)
    assert lib.vslam_rectify_build_maps(C.byref(mk()), 2, w, h, xy, fr) == pkg.VSLAM_ERR_ARG
    assert lib.vslam_rectify_build_maps(C.byref(mk()), 0, w, h, None, fr) == pkg.VSLAM_ERR_ARG


# Share of a rig's map that may sit within 1e-6 of a rounding tie.  32 u mod 1 is close to uniform on a distorted rig, so the expected share
# is 2 coordinates x 2e-6 = 4e-6; 1e-4 is 25 x that: a cap that keeps the tolerance below from hiding a wrong map.
TIE_EPS, TIE_CAP = 1e-6, 1e-4


@pytest.mark.parametrize("cam", (0, 1))
@pytest.mark.parametrize("rig", sorted(RR.RIGS))
def test_build_maps_equal_the_restatement(pkg, rig, cam):
    r = RR.RIGS[rig]
    w, h = r["dst"]
    c = r["cams"][cam]
    want_xy, want_frac = RR.build_maps(c, w, h)
    ties = RR.near_ties(c, w, h, TIE_EPS)
    print("%s cam %d: %d near-tie entries of %d (share %.2e)" % (rig, cam, ties.sum(), ties.size, ties.mean()))
    assert ties.mean() <= TIE_CAP                          # the reference alone meets the cap
    if rig == "identity":
        assert not ties.any()
    xy, frac = pkg.rectify_build_maps(RR.params_of(pkg, rig), cam, w, h)
    same = (xy == want_xy).all(axis=-1) & (frac == want_frac)
    assert same[~ties].all(), "%d entries differ away from any tie" % (~same[~ties]).sum()
    # at a near tie the fixed-point coordinate (32 * s + a) may differ by one unit, nothing more
    fix = lambda m, f: (m[..., 0].astype(np.int64) * 32 + (f & 31), m[..., 1].astype(np.int64) * 32 + (f >> 5))
    gu, gv = fix(xy, frac); wu, wv = fix(want_xy, want_frac)
    assert (np.abs(gu - wu)[ties] <= 1).all() and (np.abs(gv - wv)[ties] <= 1).all()
    print("  differing near-tie entries: %d" % (~same[ties]).sum())
