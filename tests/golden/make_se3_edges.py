"""Generator of tests/golden/se3_edges.npz: SE3 poses at the edges of csrc/se3_device.h with their exact logarithms, norms, angleY, products and
gate decisions, computed with mpmath at 60 digits.  CPU only; tests/test_se3_edges.py regenerates the arrays and compares them with the file,
tests/test_gpu_se3_edges.py reads the file.

Conventions (csrc/se3_device.h): a pose is 7 doubles, unit quaternion (x, y, z, w) then translation; a tangent is [upsilon; omega].
Every pose is built as exp(xi) in mpmath, its quaternion renormalised in mpmath, and rounded ONCE to f64.  Everything "exact" below is then computed
from the STORED f64 numbers (quaternion renormalised in mpmath: the nearest rotation), so the expected values do not carry the rounding of the pose.
log takes the rotation angle in [0, pi] (a quaternion with w < 0 is negated first), which is what Sophus' 2 atan(n / w) gives for either sign.

Arrays:
  log_T (N, 7), log_xi (N, 6), log_norm (N,), log_angle_y (N,)   rotation angles theta in THETAS about three axes, translations up to 50 m, every pose
                                                                 with both signs of the quaternion (rows 2k and 2k + 1)
  prod_a, prod_b (P,), prod_T (P, 7)                             log_T[prod_a] o log_T[prod_b], exact, rounded once (the sign the Hamilton product gives)
  gate_T (M, 7), gate_n (M,), gate_gap (M,)                      the threshold pairs: |log T| = 5 g (1 +- 1e-6) for g = 1, 2, 3 (pure translations, mixed
  gate_check (M,), gate_state (M,), gate_norm, gate_angle_y      motions and rotations one step of 1e-11 from pi), angleY = 0.03 (1 +- 1e-6) and -0.03,
                                                                 inlier counts 9, 10, 79, 80; gate_check = check_motion(n, T, gap), gate_state =
                                                                 keyframe_state(n, T) at gap 1 (0 rejected, 1 tracked, 2 keyframe); both signs again
  chain_rel (2048, 7), chain_abs (2049, 7)                       relative poses with steps up to 2 m and 0.1 rad; G_0 = identity, G_f = rel[f - 1] o G_{f-1}
                                                                 exact on the stored rel, rounded once
The 1e-6 margins are four orders above the 2e-10 the |w| < 1e-10 branch of se3::log may be off (it takes pi for 2 atan(n / w); the difference is at
most 2 |w| / n), and ten above an f64 rounding: the decisions are unambiguous for any f64 implementation.  generate() asserts the margins."""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
PI = mp.pi
THETAS = [mp.mpf(0), mp.mpf("1e-12"), mp.mpf("1e-10") * (1 - mp.mpf("1e-3")), mp.mpf("1e-10") * (1 + mp.mpf("1e-3")),
          mp.mpf("2e-10") * (1 - mp.mpf("1e-3")), mp.mpf("2e-10") * (1 + mp.mpf("1e-3")),   # (|q.xyz| = sin(theta / 2) crosses 1e-10 here)
          mp.mpf("1e-6"), mp.mpf("0.03"), mp.mpf(1), PI - mp.mpf("1e-6"), PI - mp.mpf("1e-11"), PI]
AXES = [(1, 2, 3), (-2, 1, 0.5), (0, 1, 0)]
UPSILONS = [(0.3, -0.2, 0.4), (-5, 4, 2.9), (28, -33, 25)]      # norms 0.54, 7.0, 49.9


def _vec(v):
    return [mp.mpf(x) for x in v]


def _unit(v):
    v = _vec(v); n = mp.sqrt(sum(x * x for x in v))
    return [x / n for x in v]


def _hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def exp(xi):
    """the pose of a tangent [upsilon; omega] as 7 mpf"""
    ups, om = mp.matrix(xi[:3]), list(xi[3:])
    th = mp.sqrt(sum(x * x for x in om))
    if th == 0:
        return [mp.mpf(0)] * 3 + [mp.mpf(1)] + list(ups)
    O = _hat(om)
    V = mp.eye(3) + (1 - mp.cos(th)) / th ** 2 * O + (th - mp.sin(th)) / th ** 3 * O * O
    s = mp.sin(th / 2) / th
    return [s * x for x in om] + [mp.cos(th / 2)] + list(V * ups)


def _normalised(T):
    n = mp.sqrt(sum(x * x for x in T[:4]))
    return [x / n for x in T[:4]] + list(T[4:])


def stored(T):
    """the f64 numbers a pose is stored as: quaternion renormalised, rounded once"""
    return np.array([float(x) for x in _normalised(T)], np.float64)


def exact(T64):
    """the stored f64 pose as mpf, quaternion renormalised"""
    return _normalised([mp.mpf(float(x)) for x in T64])


def rotmat(T):
    x, y, z, w = T[:4]
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def log(T):
    q = list(T[:4])
    if q[3] < 0:
        q = [-x for x in q]
    n = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    t = mp.matrix(T[4:7])
    if n == 0:
        return list(t) + [mp.mpf(0)] * 3
    th = 2 * mp.atan2(n, q[3])
    om = [th * x / n for x in q[:3]]
    O = _hat(om)
    c = (1 - th * mp.cos(th / 2) / (2 * mp.sin(th / 2))) / th ** 2
    return list((mp.eye(3) - O / 2 + c * O * O) * t) + om


def angle_y(T):
    R = rotmat(T)
    return mp.atan2(-R[2, 0], mp.sqrt(R[0, 0] ** 2 + R[1, 0] ** 2))


def mul(A, B):
    ax, ay, az, aw = A[:4]; bx, by, bz, bw = B[:4]
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
         aw * bw - ax * bx - ay * by - az * bz]
    return q + list(rotmat(A) * mp.matrix(B[4:7]) + mp.matrix(A[4:7]))


def norm(v):
    return mp.sqrt(sum(x * x for x in v))


def _both_signs(T64):
    neg = T64.copy(); neg[:4] = -neg[:4]
    return [T64, neg]


def _f(v):
    return np.array([float(x) for x in v], np.float64)


def _log_set():
    T = []
    for k, th in enumerate(THETAS):
        for a, axis in enumerate(AXES):
            xi = _vec(UPSILONS[(k + a) % 3]) + [th * x for x in _unit(axis)]
            T += _both_signs(stored(exp(xi)))
    T = np.stack(T)
    E = [exact(t) for t in T]
    xi = [log(e) for e in E]
    pa = np.arange(len(T), dtype=np.int32); pb = ((pa * 7 + 3) % len(T)).astype(np.int32)
    return dict(log_T=T, log_xi=np.stack([_f(x) for x in xi]), log_norm=_f([norm(x) for x in xi]), log_angle_y=_f([angle_y(e) for e in E]),
                prod_a=pa, prod_b=pb, prod_T=np.stack([stored(mul(E[i], E[j])) for i, j in zip(pa, pb)]))


def _quat_zyx(c, a, b):
    """Rz(c) Ry(a) Rx(b): angleY of this rotation is a for |a| < pi / 2"""
    qz = [0, 0, mp.sin(c / 2), mp.cos(c / 2), 0, 0, 0]; qy = [0, mp.sin(a / 2), 0, mp.cos(a / 2), 0, 0, 0]; qx = [mp.sin(b / 2), 0, 0, mp.cos(b / 2), 0, 0, 0]
    return mul(mul(qz, qy), qx)[:4]


def _gate_set():
    rows = []       # (pose as mpf, inliers, gap)
    pm = [1 - mp.mpf("1e-6"), 1 + mp.mpf("1e-6")]
    for g in (1, 2, 3):
        for s in pm:
            r = 5 * g * s
            rows.append((exp([r * x for x in _unit((2, -1, 2))] + [0, 0, 0]), 50, g))                       # a pure translation
            th = mp.mpf("2.5") * s                                                                             # a mixed motion: |omega| = 2.5 s
            rows.append((exp([mp.sqrt(r * r - th * th) * x for x in _unit((1, 3, -2))] + [th * x for x in _unit((3, -1, 2))]), 50, g))
            th = PI - mp.mpf("1e-11")                                                                          # |w| = 5e-12: the branch that takes pi
            rows.append((exp([mp.sqrt(r * r - th * th) * x for x in _unit((-1, 2, 2))] + [th * x for x in _unit((1, 1, -1))]), 50, g))
    for a in (mp.mpf("0.03") * pm[0], mp.mpf("0.03") * pm[1], mp.mpf("-0.03")):
        for n in (79, 80, 200):
            rows.append((_quat_zyx(mp.mpf("0.2"), a, mp.mpf("-0.1")) + _vec((0.1, 0.2, 0.3)), n, 1))
    for a in (mp.mpf("0.01"), mp.mpf("0.05")):
        for n in (9, 10, 79, 80):
            rows.append((_quat_zyx(mp.mpf("-0.3"), a, mp.mpf("0.2")) + _vec((0.5, -0.2, 0.7)), n, 1))
    T, ns, gaps = [], [], []
    for pose, n, g in rows:
        for t in _both_signs(stored(pose)):
            T.append(t); ns.append(n); gaps.append(g)
    E = [exact(t) for t in T]
    nrm = [norm(log(e)) for e in E]; ay = [angle_y(e) for e in E]
    for x, g in zip(nrm, gaps):     # no decision closer than 5e-7 relative to a threshold
        assert min(abs(x / (5 * k) - 1) for k in (1, g)) > mp.mpf("5e-7"), (x, g)
    for y in ay:
        assert abs(y / mp.mpf("0.03") - 1) > mp.mpf("5e-7"), y
    check = [n >= 10 and not x > 5 * g for x, n, g in zip(nrm, ns, gaps)]
    state = [0 if (n < 10 or x > 5) else (1 if n >= 80 and y < mp.mpf("0.03") else 2) for x, y, n in zip(nrm, ay, ns)]
    return dict(gate_T=np.stack(T), gate_n=np.array(ns, np.int32), gate_gap=np.array(gaps, np.float64), gate_check=np.array(check, np.uint8),
                gate_state=np.array(state, np.int32), gate_norm=_f(nrm), gate_angle_y=_f(ay))


def _chain_set(n=2048):
    rng = np.random.default_rng(20240)
    d = rng.normal(size=(n, 6))
    ups = d[:, :3] / np.linalg.norm(d[:, :3], axis=1, keepdims=True) * rng.uniform(0, 2.0, (n, 1))
    om = d[:, 3:] / np.linalg.norm(d[:, 3:], axis=1, keepdims=True) * rng.uniform(0, 0.1, (n, 1))
    rel = np.stack([stored(exp(_vec(np.concatenate([u, o]).tolist()))) for u, o in zip(ups, om)])
    G = [[mp.mpf(0)] * 3 + [mp.mpf(1)] + [mp.mpf(0)] * 3]
    for r in rel:
        G.append(_normalised(mul(exact(r), G[-1])))
    return dict(chain_rel=rel, chain_abs=np.stack([stored(g) for g in G]))


def generate():
    out = {}
    for part in (_log_set(), _gate_set(), _chain_set()):
        out.update(part)
    return out


if __name__ == "__main__":
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "se3_edges.npz"), **generate())
