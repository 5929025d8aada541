"""The numpy yardstick of the pose-graph stage (include/vslam_hip.h "pose-graph optimisation"; the reference has no pose graph, so nothing is ported).

Problem: node k holds T_k = T_c_w (quaternion x, y, z, w then translation); an edge (i, j, Z, w) has the residual r = log(Z^-1 T_i T_j^-1) and the
cost r' diag(w) r; update T <- exp(delta) T; with E = Z^-1 T_i T_j^-1 and A = I - ad(r)/2 + ad(r)^2/12 the Jacobians are A Ad(Z^-1) and -A Ad(E).
Levenberg-Marquardt on H + lambda diag(H) from lambda 1e-4, /10 on an accepted step (floor 1e-12), x10 on a rejected one, stop at |delta| < step_tol,
lambda > 1e12 or max_iters.  Held nodes: the fixed ones (default node 0) and those without an active edge.

solve(mode="dense") solves every step exactly; solve(mode="pcg") runs preconditioned conjugate gradients with the block-Jacobi (precond 0) or the
chain (block-tridiagonal, precond 1) preconditioner at the library's default parameters.  cost_and_gradient() walks the edges once, O(E), no matrix.
The SE3 functions restate csrc/se3_device.h (Sophus' exp / log)."""
import numpy as np

EPS = 1e-10
DEFAULTS = dict(max_iters=50, pcg_max_iters=4000, pcg_tol=1e-10, step_tol=1e-9, lambda_init=1e-4)


# ------------------------------------------------------------------------------------------ SE3, vectorised over the leading axis
def rotmat(T):
    x, y, z, w = T[..., 0], T[..., 1], T[..., 2], T[..., 3]
    R = np.empty(T.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def mul(A, B):
    ax, ay, az, aw = (A[..., k] for k in range(4)); bx, by, bz, bw = (B[..., k] for k in range(4))
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz], -1)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    t = np.einsum("...ij,...j->...i", rotmat(A), B[..., 4:]) + A[..., 4:]
    return np.concatenate([q, t], -1)


def inverse(A):
    q = A[..., :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    t = -np.einsum("...ji,...j->...i", rotmat(A), A[..., 4:])
    return np.concatenate([q, t], -1)


def hat(v):
    M = np.zeros(v.shape[:-1] + (3, 3))
    M[..., 0, 1] = -v[..., 2]; M[..., 0, 2] = v[..., 1]; M[..., 1, 0] = v[..., 2]
    M[..., 1, 2] = -v[..., 0]; M[..., 2, 0] = -v[..., 1]; M[..., 2, 1] = v[..., 0]
    return M


def exp(xi):
    xi = np.asarray(xi, np.float64)
    ups, om = xi[..., :3], xi[..., 3:]
    th2 = (om * om).sum(-1); th = np.sqrt(th2); small = th < EPS
    ths = np.where(small, 1.0, th)
    imag = np.where(small, 0.5 - th2 / 48.0 + th2 * th2 / 3840.0, np.sin(0.5 * ths) / ths)
    real = np.where(small, 1.0 - th2 / 8.0 + th2 * th2 / 384.0, np.cos(0.5 * ths))
    q = np.concatenate([imag[..., None] * om, real[..., None]], -1)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    O = hat(om); O2 = O @ O
    a = np.where(small, 0.5, (1 - np.cos(ths)) / (ths * ths)); b = np.where(small, 1.0 / 6.0, (ths - np.sin(ths)) / (ths ** 3))
    V = np.eye(3) + a[..., None, None] * O + b[..., None, None] * O2
    return np.concatenate([q, np.einsum("...ij,...j->...i", V, ups)], -1)


def log(T):
    v, w = T[..., :3], T[..., 3]
    sq = (v * v).sum(-1); n = np.sqrt(sq)
    ns = np.where(n < EPS, 1.0, n); wsafe = np.where(np.abs(w) < EPS, 1.0, w)
    two_atan = np.where(n < EPS, 2.0 / wsafe - 2.0 * sq / wsafe ** 3, np.where(np.abs(w) < EPS, np.where(w > 0, np.pi, -np.pi) / ns, 2.0 * np.arctan(n / wsafe) / ns))
    om = two_atan[..., None] * v
    th = two_atan * n; small = np.abs(th) < EPS
    ths = np.where(small, 1.0, th)
    c = np.where(small, 1.0 / 12.0, (1.0 - ths * np.cos(0.5 * ths) / (2.0 * np.sin(0.5 * ths))) / (ths * ths))
    O = hat(om)
    Vi = np.eye(3) - 0.5 * O + c[..., None, None] * (O @ O)
    return np.concatenate([np.einsum("...ij,...j->...i", Vi, T[..., 4:]), om], -1)


def Ad(T):
    R = rotmat(T)
    M = np.zeros(T.shape[:-1] + (6, 6))
    M[..., :3, :3] = R; M[..., 3:, 3:] = R; M[..., :3, 3:] = hat(T[..., 4:]) @ R
    return M


def ad(r):
    M = np.zeros(r.shape[:-1] + (6, 6))
    O = hat(r[..., 3:])
    M[..., :3, :3] = O; M[..., 3:, 3:] = O; M[..., :3, 3:] = hat(r[..., :3])
    return M


# ------------------------------------------------------------------------------------------ the problem
def residuals(T, ei, ej, Z):
    """(r (E, 6), E, Z^-1)"""
    Zi = inverse(Z)
    Em = mul(Zi, mul(T[ei], inverse(T[ej])))
    return log(Em), Em, Zi


def jacobians(r, Em, Zi, exact_A=True):
    """(dr/d delta_i, dr/d delta_j), each (E, 6, 6); exact_A False drops the factor A (the shortcut the design rejects)"""
    a = ad(r)
    A = np.eye(6) - 0.5 * a + (a @ a) / 12.0 if exact_A else np.broadcast_to(np.eye(6), a.shape)
    return A @ Ad(Zi), -(A @ Ad(Em))


def held_nodes(N, ei, ej, fixed, active):
    held = np.zeros(N, bool)
    if fixed is None:
        held[:1] = True
    else:
        held |= np.asarray(fixed).astype(bool)
    deg = np.zeros(N, np.int64)
    np.add.at(deg, ei[active], 1); np.add.at(deg, ej[active], 1)
    return held | (deg == 0)


def _active(E, active):
    return np.ones(E, bool) if active is None else np.asarray(active).astype(bool)


def edge_chi2(T, ei, ej, Z, w):
    r = residuals(T, ei, ej, Z)[0]
    return (r * w * r).sum(-1)


def cost_and_gradient(T, ei, ej, Z, w, fixed=None, active=None):
    """(cost, g (N, 6)) of the active edges, g_n = sum J' W r over the edges at node n (the gradient of cost / 2 under T <- exp(delta) T), zero at held
    nodes; one pass over the edges"""
    T = np.asarray(T, np.float64); N, E = len(T), len(ei)
    act = _active(E, active)
    ei, ej, Z, w = ei[act], ej[act], Z[act], w[act]
    r, Em, Zi = residuals(T, ei, ej, Z)
    Ji, Jj = jacobians(r, Em, Zi)
    wr = w * r
    g = np.zeros((N, 6))
    np.add.at(g, ei, np.einsum("eij,ei->ej", Ji, wr)); np.add.at(g, ej, np.einsum("eij,ei->ej", Jj, wr))
    g[held_nodes(N, ei, ej, fixed, np.ones(len(ei), bool))] = 0
    return float((r * wr).sum()), g


def _system(T, ei, ej, Z, w, N):
    r, Em, Zi = residuals(T, ei, ej, Z)
    Ji, Jj = jacobians(r, Em, Zi)
    H = np.zeros((N, 6, N, 6)); b = np.zeros((N, 6))
    WJi, WJj = w[:, :, None] * Ji, w[:, :, None] * Jj
    for e in range(len(ei)):
        i, j = ei[e], ej[e]
        H[i, :, i, :] += Ji[e].T @ WJi[e]; H[j, :, j, :] += Jj[e].T @ WJj[e]
        H[i, :, j, :] += Ji[e].T @ WJj[e]; H[j, :, i, :] += Jj[e].T @ WJi[e]
        b[i] -= Ji[e].T @ (w[e] * r[e]); b[j] -= Jj[e].T @ (w[e] * r[e])
    return H.reshape(6 * N, 6 * N), b.reshape(-1), float((r * w * r).sum())


def _pcg(Hd, b, nodes, precond, tol, max_iters):
    """PCG on Hd x = b over the free nodes `nodes` (their ids: the chain preconditioner couples consecutive ids only); returns (x, iterations)"""
    n = len(b)
    M = np.zeros_like(Hd)
    for a in range(len(nodes)):
        sa = slice(6 * a, 6 * a + 6)
        M[sa, sa] = Hd[sa, sa]
        if precond == 1 and a + 1 < len(nodes) and nodes[a + 1] == nodes[a] + 1:
            sb = slice(6 * a + 6, 6 * a + 12)
            M[sa, sb] = Hd[sa, sb]; M[sb, sa] = Hd[sb, sa]
    Minv = np.linalg.inv(M)
    x = np.zeros(n); r = b.copy(); z = Minv @ r; p = z.copy(); rz = r @ z; rr0 = rr = r @ r
    it = 0
    while rr0 > 0 and rr > tol * tol * rr0 and it < max_iters:
        y = Hd @ p
        py = p @ y
        if not py > 0:
            break
        alpha = rz / py
        x += alpha * p; r -= alpha * y
        z = Minv @ r
        rz_new = r @ z; rr = r @ r
        p = z + (rz_new / rz) * p; rz = rz_new
        it += 1
    return x, it


def solve(T, ei, ej, Z, w, fixed=None, active=None, mode="dense", precond=0, polish=0, **params):
    """Levenberg-Marquardt as the module docstring states it.  Returns dict(T, chi2_init, chi2_final, lm_iters, pcg_iters, lam, n_free).
    polish: up to that many undamped Gauss-Newton steps afterwards, each kept when the gradient norm falls.  The cost test of LM rejects steps once the
    cost changes by less than its own rounding, which on a weakly tied graph (one loop edge on a long ring) is while the poses still move by 1e-9;
    the gradient can be driven to its rounding floor.  For the yardstick's converged poses only: the library has no such phase."""
    P = dict(DEFAULTS); P.update(params)
    T = np.array(T, np.float64).reshape(-1, 7); N = len(T)
    ei = np.asarray(ei, np.int64); ej = np.asarray(ej, np.int64); Z = np.asarray(Z, np.float64).reshape(-1, 7); w = np.asarray(w, np.float64).reshape(-1, 6)
    act = _active(len(ei), active)
    ei, ej, Z, w = ei[act], ej[act], Z[act], w[act]
    free = ~held_nodes(N, ei, ej, fixed, np.ones(len(ei), bool))
    nodes = np.nonzero(free)[0]
    dof = (nodes[:, None] * 6 + np.arange(6)).ravel()
    cost = float(edge_chi2(T, ei, ej, Z, w).sum()) if len(ei) else 0.0
    out = dict(chi2_init=cost, lm_iters=0, pcg_iters=0, n_free=int(free.sum()))
    lam, fresh = P["lambda_init"], True
    for it in range(P["max_iters"] if len(nodes) else 0):
        if fresh:
            H, b, _ = _system(T, ei, ej, Z, w, N)
            H, b = H[np.ix_(dof, dof)], b[dof]
            fresh = False
        Hd = H + lam * np.diag(np.diag(H))
        if mode == "dense":
            x = np.linalg.solve(Hd, b)
        else:
            x, n_it = _pcg(Hd, b, nodes, precond, P["pcg_tol"], P["pcg_max_iters"])
            out["pcg_iters"] += n_it
        Tn = T.copy()
        Tn[nodes] = mul(exp(x.reshape(-1, 6)), T[nodes])
        cost_new = float(edge_chi2(Tn, ei, ej, Z, w).sum())
        out["lm_iters"] = it + 1
        if cost_new < cost:
            T, cost, fresh, lam = Tn, cost_new, True, max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        if not np.linalg.norm(x) >= P["step_tol"] or lam > 1e12:
            break
    for _ in range(polish if len(nodes) else 0):
        H, b, _ = _system(T, ei, ej, Z, w, N)
        Tn = T.copy()
        Tn[nodes] = mul(exp(np.linalg.solve(H[np.ix_(dof, dof)], b[dof]).reshape(-1, 6)), T[nodes])
        if not np.linalg.norm(_system(Tn, ei, ej, Z, w, N)[1][dof]) < np.linalg.norm(b[dof]):
            break
        T = Tn
    if polish and len(ei):
        cost = float(edge_chi2(T, ei, ej, Z, w).sum())
    out.update(T=T, chi2_final=cost, lam=lam)
    return out
