"""CPU: tests/golden/se3_edges.npz is what tests/golden/make_se3_edges.py writes; the host entry vslam_check_motion decides every threshold pair as
mpmath does; and the numpy restatement of se3::log (tests/pose_graph_ref.py) meets, on the CPU, the tolerances tests/test_gpu_se3_edges.py asks of
the device -- so those tolerances are known to be attainable by f64 arithmetic of the same formulas before a GPU sees them."""
import ctypes as C
import importlib.util
import os

import numpy as np

import pose_graph_ref as R
import se3_edges_cases as Cs


def test_golden_file_regenerates():
    spec = importlib.util.spec_from_file_location("make_se3_edges", os.path.join(os.path.dirname(Cs.PATH), "make_se3_edges.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    fresh, kept = mod.generate(), Cs.load()
    assert sorted(fresh) == sorted(kept)
    for k in kept:
        assert fresh[k].dtype == kept[k].dtype and fresh[k].shape == kept[k].shape and fresh[k].tobytes() == kept[k].tobytes(), k


def test_vectors_cover_the_branches():
    d = Cs.load()
    T = d["log_T"]
    n = np.linalg.norm(T[:, :3], axis=1)
    assert (n < 1e-10).sum() >= 12 and ((np.abs(T[:, 3]) < 1e-10) & (n >= 1e-10)).sum() >= 12 and (T[:, 3] < 0).sum() == len(T) // 2
    th = np.linalg.norm(d["log_xi"][:, 3:], axis=1)
    assert ((th > 0) & (th < 1e-10)).any() and ((th > 1e-10) & (th < 1.01e-10)).any()        # either side of the c = 1/12 switch
    assert np.array_equal(T[0::2, :4], -T[1::2, :4]) and np.array_equal(d["log_xi"][0::2], d["log_xi"][1::2])
    assert np.abs(np.linalg.norm(d["chain_abs"][:, :4], axis=1) - 1).max() <= 2 * Cs.EPS
    assert set(d["gate_state"].tolist()) == {0, 1, 2} and 0 < d["gate_check"].sum() < len(d["gate_check"])


def test_check_motion_host_decisions(pkg):
    """vslam_check_motion is host arithmetic: every threshold pair, both quaternion signs, at the pair's own frame gap"""
    d = Cs.load()
    lib = pkg.load_library()
    got = [lib.vslam_check_motion(int(n), np.ascontiguousarray(T).ctypes.data_as(C.c_void_p), C.c_double(g)) for T, n, g in zip(d["gate_T"], d["gate_n"], d["gate_gap"])]
    assert got == d["gate_check"].tolist()


def test_numpy_restatement_meets_the_device_tolerances():
    d = Cs.load()
    T, xi = d["log_T"], d["log_xi"]
    Z = np.tile(Cs.IDENT, (len(T), 1))
    r = R.log(R.mul(R.inverse(Z), R.mul(T, R.inverse(Z))))        # the edge residual of a two-node graph: node 0 at identity, node 1 = T, Z = identity
    err = np.abs(np.abs(r) - np.abs(xi)).max(axis=1)
    tol = Cs.log_tolerance(T, xi)
    print("numpy log vs mpmath: worst error / tolerance %.3g, worst error %.3g (|w| < 1e-10: %.3g)" % ((err / tol).max(), err.max(), err[np.abs(T[:, 3]) < 1e-10].max()))
    assert (err <= tol).all(), np.flatnonzero(err > tol)
    assert np.abs(np.linalg.norm(r, axis=1) - d["log_norm"]).max() <= tol.max()
    P = R.mul(T[d["prod_a"]], T[d["prod_b"]])
    dq = np.minimum(np.linalg.norm(P[:, :4] - d["prod_T"][:, :4], axis=1), np.linalg.norm(P[:, :4] + d["prod_T"][:, :4], axis=1))
    assert dq.max() <= 8 * Cs.EPS and np.abs(P[:, 4:] - d["prod_T"][:, 4:]).max() <= 64 * Cs.EPS * 100
    eq, et, en = Cs.chain_errors(Cs.numpy_chain(d["chain_rel"]), d["chain_abs"])
    print("numpy chain vs mpmath: quaternion %.3g, translation %.3g, | |q| - 1 | %.3g" % (eq, et, en))
    assert en <= 4 * Cs.EPS and 0 < eq < 1e-12 and 0 < et < 1e-9
