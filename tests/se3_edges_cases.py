"""What tests/test_se3_edges.py (CPU) and tests/test_gpu_se3_edges.py share: the stored vectors of tests/golden/se3_edges.npz (written by
tests/golden/make_se3_edges.py with mpmath), the tolerance of a computed logarithm against them, and the error measures of a pose chain."""
import os

import numpy as np

import pose_graph_ref as R

EPS = np.finfo(np.float64).eps
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se3_edges.npz")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def load():
    with np.load(PATH) as d:
        return {k: d[k] for k in d.files}


def log_tolerance(T, xi):
    """per pose: 4e-10 absolute where |w| < 1e-10 -- se3::log takes pi for 2 atan(n / w) there, off by at most 2 |w| / n <= 2e-10 -- and
    64 eps max(1, |xi|) on every other branch"""
    return np.where(np.abs(T[:, 3]) < 1e-10, 4e-10, 64 * EPS * np.maximum(1.0, np.linalg.norm(xi, axis=1)))


def numpy_chain(rel):
    """G_0 = identity, G_f = rel[f - 1] o G_{f - 1}, one after the other in numpy f64 (tests/pose_graph_ref.py's product)"""
    G = [IDENT.copy()]
    for r in rel:
        G.append(R.mul(r, G[-1]))
    return np.stack(G)


def chain_errors(G, want):
    """(max quaternion error up to the sign of q, max translation error, max | |q| - 1 |) of a chain against the exact one"""
    dq = np.minimum(np.linalg.norm(G[:, :4] - want[:, :4], axis=1), np.linalg.norm(G[:, :4] + want[:, :4], axis=1))
    return float(dq.max()), float(np.linalg.norm(G[:, 4:] - want[:, 4:], axis=1).max()), float(np.abs(np.linalg.norm(G[:, :4], axis=1) - 1).max())
