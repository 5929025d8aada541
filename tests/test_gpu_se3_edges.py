"""GPU: the SE3 arithmetic of csrc/se3_device.h behind the motion gate, the keyframe gate, the pose chain and the pose-graph residual, against
values computed with mpmath at 60 digits (tests/golden/se3_edges.npz, written by tests/golden/make_se3_edges.py) instead of against restatements of
the same branches.  The vectors sit on every branch of se3::log -- |q.xyz| < 1e-10, |w| < 1e-10, the general one with w of either sign, and both
sides of the c = 1/12 switch -- with translations up to 50 m, and one relative step of 1e-6 on either side of every threshold of the gates."""
import ctypes as C

import numpy as np
import pytest

import se3_edges_cases as Cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vec():
    return Cs.load()


def _gate(vo, T, absolute, ninl):
    import torch
    F = len(ninl) + 1
    tT = torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda(); tn = torch.from_numpy(np.ascontiguousarray(ninl, np.int32)).cuda()
    st = torch.full((F,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vo.gate_states_dev(F, tT.data_ptr(), absolute, tn.data_ptr(), st.data_ptr())
    vo.sync()
    return st.cpu().numpy()


def test_gate_decisions(vo, vec):
    """vslam_check_motion (host, at each pair's own frame gap) and vslam_gate_states_dev (device, frame gap 1, on relative and on absolute poses)
    decide every threshold pair as mpmath does, for both signs of the quaternion.  absolute = 1 takes T_c_l = G_f o G_{f-1}^-1: the poses are laid
    out as G = (I, T_0, I, T_1, ...), so every odd frame sees T_k o I (the even ones see the inverses and are not judged)."""
    T, n = vec["gate_T"], vec["gate_n"]
    host = [vo.lib.vslam_check_motion(int(k), np.ascontiguousarray(t).ctypes.data_as(C.c_void_p), C.c_double(g)) for t, k, g in zip(T, n, vec["gate_gap"])]
    assert host == vec["gate_check"].tolist()
    want = vec["gate_state"]
    rel = _gate(vo, T, 0, n)
    assert rel[0] == 2 and np.array_equal(rel[1:], want)
    G = np.tile(Cs.IDENT, (2 * len(T) + 1, 1)); G[1::2] = T
    ab = _gate(vo, G, 1, np.repeat(n, 2))
    assert ab[0] == 2 and np.array_equal(ab[1::2], want)


def test_device_log_components(vo, vec):
    """se3::log on the device, component by component: vslam_pose_graph_dev with max_iters = 0 evaluates r = log(Z^-1 T_i T_j^-1) per edge.  One
    graph per pose: node 0 at identity, node 1 = T, six edges (i, j) = (1, 0) with Z = identity and the six one-hot weight vectors, so the edge
    chi2 are r_k^2 with r = log(T o I) = xi itself (no sign flip, no adjoint: i is the moved node).  sqrt(chi2_k) against |xi_k| from mpmath.
    Tolerance (Cs.log_tolerance): 4e-10 where |w| < 1e-10, 64 eps max(1, |xi|) elsewhere.  The numpy restatement of the same formulas, measured
    against the same vectors on the CPU (tests/test_se3_edges.py), is within 0.50 of that tolerance everywhere (worst 1.98e-10, in the |w| < 1e-10
    branch at theta = pi - 1e-11 with a 50 m translation), so the tolerance stands as derived; the device measures the same 0.50 / 1.98e-10."""
    T, xi = vec["log_T"], vec["log_xi"]
    N = len(T)
    nodes = np.tile(Cs.IDENT, (2 * N, 1)); nodes[1::2] = T
    E = 6 * N
    edges = dict(off=np.arange(N + 1, dtype=np.int32) * 6, i=np.ones(E, np.int32), j=np.zeros(E, np.int32), Z=np.tile(Cs.IDENT, (E, 1)),
                 w=np.tile(np.eye(6), (N, 1)))
    out = vo.optimize_pose_graph(nodes, np.arange(N + 1, dtype=np.int32) * 2, edges, max_iters=0)
    assert np.array_equal(out["T"], nodes)
    got = np.sqrt(out["edge_chi2"].reshape(N, 6))
    err = np.abs(got - np.abs(xi)).max(axis=1)
    tol = Cs.log_tolerance(T, xi)
    print("device log vs mpmath: worst error / tolerance %.3g, worst error %.3g" % ((err / tol).max(), err.max()))
    assert (err <= tol).all(), (np.flatnonzero(err > tol), err[err > tol])
    assert np.abs(np.sqrt(out["edge_chi2"].reshape(N, 6).sum(1)) - vec["log_norm"]).max() <= tol.max()


def test_chain_against_exact(vo, vec):
    """vslam_chain_poses_dev on 2048 relative poses (2049 frames: nine 256-frame rounds of its scan) against the exact absolute poses, up to the sign
    of q.  Bound: 4 x the error of the sequential numpy-f64 chain against the same exact poses, computed here (on the CPU it measures 7.8e-15 on
    the quaternion and 3.8e-13 m on the translation after 2048 steps); both chains round once per product, the factor covers the order of the
    products (the device scans in a tree; it measures 7.2e-16 and 7.9e-14 m).  Every quaternion is unit to 4 eps."""
    import torch
    rel, want = vec["chain_rel"], vec["chain_abs"]
    F = len(want)
    tr = torch.from_numpy(rel).cuda(); tG = torch.full((F, 7), -3.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vo.chain_poses_dev(F, tr.data_ptr(), tG.data_ptr())
    vo.sync()
    G = tG.cpu().numpy()
    rq, rt, _ = Cs.chain_errors(Cs.numpy_chain(rel), want)
    gq, gt, gn = Cs.chain_errors(G, want)
    print("chain vs mpmath: device q %.3g t %.3g | |q| - 1 | %.3g; numpy q %.3g t %.3g" % (gq, gt, gn, rq, rt))
    assert gn <= 4 * Cs.EPS
    assert gq <= 4 * rq and gt <= 4 * rt
