"""tests/glue_ref.py on tables small enough to work by hand: the expected values below are written out, not computed."""
import numpy as np

import glue_ref as R


def _kps(pkg, xy):
    k = np.zeros(len(xy), pkg.KEYPOINT_DTYPE)
    k["x"] = [p[0] for p in xy]; k["y"] = [p[1] for p in xy]
    return k


def _matches(pkg, qt, capacity=None):
    m = np.zeros(len(qt) if capacity is None else capacity, pkg.DMATCH_DTYPE)
    m["queryIdx"][:len(qt)] = [p[0] for p in qt]; m["trainIdx"][:len(qt)] = [p[1] for p in qt]
    return m


def test_gather_uv_by_hand(pkg):
    kQ = _kps(pkg, [(10, 11), (20, 21), (30, 31)]); kT = _kps(pkg, [(1.5, 2.5), (3.5, 4.5), (5.5, 6.5)])
    m = _matches(pkg, [(0, 2), (5, -1), (1, 1)])
    rows, q, t = R.gather_uv(kQ, kT, m, 7, 3)              # a count above the capacity: the capacity
    assert rows == 3
    assert q.tolist() == [[10, 11], [30, 31], [20, 21]]    # 5 clamps to keypoint 2
    assert t.tolist() == [[5.5, 6.5], [1.5, 2.5], [3.5, 4.5]]   # -1 clamps to keypoint 0
    rows, q, t = R.gather_uv(kQ, kT, m, 2, 3)
    assert rows == 2 and q.tolist() == [[10, 11], [30, 31]] and t.tolist() == [[5.5, 6.5], [1.5, 2.5]]
    for n in (0, -3):
        rows, q, t = R.gather_uv(kQ, kT, m, n, 3)
        assert rows == 0 and q.shape == (0, 2) and t.shape == (0, 2)


def test_build_pnp_inputs_by_hand(pkg):
    """four keypoints; L/R matches with queryIdx 2, 0, 2, 7: keypoint 2 occurs twice (the later match, 2, wins) and 7 is out of range"""
    lr = _matches(pkg, [(2, 0), (0, 0), (2, 0), (7, 0)])
    xyz_lr = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]], np.float32)
    valid = np.array([0, 1, 1, 1], np.uint8)              # the FIRST match of keypoint 2 is invalid: only "last wins" lets it through
    cur = _kps(pkg, [(100, 101), (110, 111), (120, 121), (130, 131)])
    f2f = _matches(pkg, [(2, 1), (1, 0), (0, 3), (-1, 2), (0, 4)])
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, 5, 5, lr, 4, 4, xyz_lr, valid, cur, 2)
    assert kp2lr.tolist() == [1, -1, 2, -1]
    # (2,1): L/R match 2, valid -> survivor 0.  (1,0): keypoint 1 has no depth.  (0,3): L/R match 1 -> survivor 1.  (-1,2), (0,4): out of range
    assert nout == 2 and xyz.tolist() == [[3, 3, 3], [2, 2, 2]] and uv.tolist() == [[110, 111], [130, 131]]
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, 5, 5, lr, 4, 4, xyz_lr, valid, cur, 1)     # the cut: two survivors, room for one
    assert nout == 1 and xyz.tolist() == [[3, 3, 3]] and uv.tolist() == [[110, 111]]
    # the L/R count cut to two: keypoint 2 falls back to match 0, which is invalid
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, 5, 5, lr, 2, 4, xyz_lr, valid, cur, 2)
    assert kp2lr.tolist() == [1, -1, 0, -1] and nout == 1 and xyz.tolist() == [[2, 2, 2]] and uv.tolist() == [[130, 131]]


def test_build_pnp_inputs_counts_by_hand(pkg):
    """counts above their capacity and below zero; three survivors into two slots"""
    lr = _matches(pkg, [(0, 0), (1, 0), (2, 0)])
    xyz_lr = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32)
    valid = np.ones(3, np.uint8)
    cur = _kps(pkg, [(7, 8), (9, 10), (11, 12)])
    f2f = _matches(pkg, [(2, 2), (1, 1), (0, 0)])
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, 9, 3, lr, 900, 3, xyz_lr, valid, cur, 2)   # 9 > 3 matches, 900 > 3 L/R matches
    assert kp2lr.tolist() == [0, 1, 2] and nout == 2 and xyz.tolist() == [[3, 0, 0], [2, 0, 0]] and uv.tolist() == [[11, 12], [9, 10]]
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, -3, 3, lr, 3, 3, xyz_lr, valid, cur, 2)
    assert kp2lr.tolist() == [0, 1, 2] and nout == 0 and xyz.shape == (0, 3) and uv.shape == (0, 2)
    kp2lr, nout, xyz, uv = R.build_pnp_inputs(f2f, 3, 3, lr, -3, 3, xyz_lr, valid, cur, 2)
    assert kp2lr.tolist() == [-1, -1, -1] and nout == 0
