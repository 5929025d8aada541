"""The numpy yardstick of the full bundle adjustment stage (include/vslam_hip.h "full bundle adjustment"; the reference has no such stage, so nothing
is ported).

A problem is a dict: T (N, 7) poses T_c_w, X (M, 3) landmarks, kf / lm (O) ids with the observations sorted by landmark, uv (O, 2) f32, disp (O) f32
or None (negative or NaN: a left-image-only observation), ei / ej / Z / w the pose-pose edges of tests/pose_graph_ref.py, fixed (N bytes or None:
keyframe 0), obs_active / edge_active (bytes or None), K4 = (fx, fy, cx, cy), bf, huber (0: none).

Residual of an observation with P = R_k X_l + t_k: e = [u - (fx Px / Pz + cx), v - (fy Py / Pz + cy)] and, with a valid disparity, d - bf / Pz.  With
A = de/dP the Jacobians are Jp = A [I, -P^] (update T <- exp(delta) T, delta = [upsilon; omega]) and Jl = A R_k.  Huber on s = e'e: rho = s for
s <= delta^2, else 2 sqrt(s) delta - delta^2; the weight rho' multiplies J'J and J'e.  Cost = sum rho over the active observations + sum r' diag(w) r
over the active edges.  An observation with Pz <= 0 at the input state is inactive for the whole call; a trial state with Pz <= 0 at an active one
costs infinity.  Held keyframes: the fixed ones and those without an active observation and without an active edge.  A landmark without an active
observation does not move; one whose damped 3 x 3 block is not positive definite is held for that iteration.

Levenberg-Marquardt exactly as tests/pose_graph_ref.py: (H + lambda diag(H)) on the full system, /10 (floor 1e-12) on a step that lowers the cost,
x10 otherwise, stop at |delta| < step_tol (poses and points together), lambda > 1e12 or max_iters.  Every step eliminates the landmarks;
solve(mode="dense") then solves the reduced camera system exactly, solve(mode="pcg") by conjugate gradients with the block-Jacobi preconditioner
(the 6 x 6 diagonal blocks of the reduced system) at the library's default parameters.  full_step() solves the undivided system for the test that
the elimination changes nothing."""
import numpy as np

import pose_graph_ref as PG

DEFAULTS = dict(max_iters=50, pcg_max_iters=4000, pcg_tol=1e-10, step_tol=1e-9, lambda_init=1e-4)
# the yardstick's converged state: past the library's default stop and polished to the rounding floor of the gradient (pose_graph_cases.CONVERGED)
CONVERGED = dict(step_tol=1e-13, max_iters=100, polish=5)
FBA_BAD_INDEX, FBA_NONFINITE, FBA_PCG_CAP, FBA_LAMBDA, FBA_SINGULAR, FBA_DROPPED = 1, 2, 4, 8, 16, 32


def _mask(n, m):
    return np.ones(n, bool) if m is None else np.asarray(m).astype(bool)


def stereo_mask(p):
    O = len(p["kf"])
    if p.get("disp") is None:
        return np.zeros(O, bool)
    d = np.asarray(p["disp"], np.float32)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(d) & (d >= 0)


def camera_points(T, X, p):
    T = np.asarray(T, np.float64); X = np.asarray(X, np.float64)
    return np.einsum("oij,oj->oi", PG.rotmat(T[p["kf"]]), X[p["lm"]]) + T[p["kf"], 4:]


def input_active(p):
    """(active observations of the call, number dropped behind the camera): decided once, at the problem's own input state"""
    act = _mask(len(p["kf"]), p.get("obs_active"))
    if len(act) == 0:
        return act, 0
    front = camera_points(p["T"], p["X"], p)[:, 2] > 0
    return act & front, int((act & ~front).sum())


def held_keyframes(p, oact=None):
    N = len(p["T"])
    oact = input_active(p)[0] if oact is None else oact
    eact = _mask(len(p["ei"]), p.get("edge_active"))
    held = np.zeros(N, bool)
    if p.get("fixed") is None:
        held[:1] = True
    else:
        held |= np.asarray(p["fixed"]).astype(bool)
    deg = np.zeros(N, np.int64)
    np.add.at(deg, p["kf"][oact], 1); np.add.at(deg, p["ei"][eact], 1); np.add.at(deg, p["ej"][eact], 1)
    return held | (deg == 0)


def residuals(T, X, p, jac=False):
    """e (O, 3) with a zero third row at mono observations; with jac also (A (O, 3, 3), P (O, 3))"""
    fx, fy, cx, cy = p["K4"]; bf = p["bf"]
    P = camera_points(T, X, p)
    O = len(P)
    st = stereo_mask(p)
    uv = np.asarray(p["uv"], np.float32).astype(np.float64).reshape(-1, 2)
    d = np.where(st, np.asarray(p["disp"], np.float32).astype(np.float64), 0.0) if p.get("disp") is not None else np.zeros(O)
    with np.errstate(all="ignore"):
        iz = 1.0 / P[:, 2]
        e = np.stack([uv[:, 0] - (fx * P[:, 0] * iz + cx), uv[:, 1] - (fy * P[:, 1] * iz + cy), np.where(st, d - bf * iz, 0.0)], -1)
        if not jac:
            return e
        A = np.zeros((O, 3, 3))
        A[:, 0, 0] = -fx * iz; A[:, 0, 2] = fx * P[:, 0] * iz * iz
        A[:, 1, 1] = -fy * iz; A[:, 1, 2] = fy * P[:, 1] * iz * iz
        A[:, 2, 2] = np.where(st, bf * iz * iz, 0.0)
    return e, A, P


def huber(s, delta):
    """(rho, rho') of oracle/lm.c huber(); delta 0: none"""
    if not delta > 0:
        return s, np.ones_like(s)
    d2 = delta * delta
    big = s > d2
    r = np.sqrt(np.where(big, s, 1.0))
    return np.where(big, 2 * r * delta - d2, s), np.where(big, delta / r, 1.0)


def obs_chi2(T, X, p):
    e = residuals(T, X, p)
    return (e * e).sum(-1)


def _edge_cost(T, p):
    eact = _mask(len(p["ei"]), p.get("edge_active"))
    if not eact.any():
        return 0.0
    return float(PG.edge_chi2(np.asarray(T, np.float64), p["ei"][eact], p["ej"][eact], p["Z"][eact], p["w"][eact]).sum())


def cost(T, X, p, oact=None):
    """the cost of a state; infinity when an active observation lies at Pz <= 0"""
    oact = input_active(p)[0] if oact is None else oact
    c = 0.0
    if oact.any():
        if (camera_points(T, X, p)[oact, 2] <= 0).any():
            return float("inf")
        c = float(huber(obs_chi2(T, X, p)[oact], p["huber"])[0].sum())
    return c + _edge_cost(T, p)


def _edge_system(T, p):
    """(H (6N, 6N), b (6N)) of the active pose-pose edges"""
    N = len(T)
    eact = _mask(len(p["ei"]), p.get("edge_active"))
    if not eact.any():
        return np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
    H, b, _ = PG._system(np.asarray(T, np.float64), np.asarray(p["ei"], np.int64)[eact], np.asarray(p["ej"], np.int64)[eact], p["Z"][eact], p["w"][eact], N)
    return H, b


def cost_and_gradient(T, X, p, oact=None):
    """(cost, gT (N, 6), gX (M, 3)): g = sum J' rho' e (the gradient of cost / 2), zero at held keyframes and at landmarks without an active
    observation"""
    T = np.asarray(T, np.float64); X = np.asarray(X, np.float64)
    oact = input_active(p)[0] if oact is None else oact
    N, M = len(T), len(X)
    gT = np.zeros((N, 6)); gX = np.zeros((M, 3))
    if oact.any():
        e, A, P = residuals(T, X, p, jac=True)
        w = huber((e * e).sum(-1), p["huber"])[1]
        g3 = np.einsum("oij,oi->oj", A, e * w[:, None])[oact]           # A' w e
        kf, lm = p["kf"][oact], p["lm"][oact]
        np.add.at(gT, kf, np.concatenate([g3, np.cross(P[oact], g3)], -1))   # [I; P^] g3
        np.add.at(gX, lm, np.einsum("oji,oj->oi", PG.rotmat(T[kf]), g3))
    gT -= _edge_system(T, p)[1].reshape(N, 6)
    gT[held_keyframes(p, oact)] = 0
    return cost(T, X, p, oact), gT, gX


def system(T, X, p, oact):
    """the blocks of the normal equations at a state: dict(Hpp (6N, 6N) with the edges, W (6N, 3M), V (M, 3, 3), bp (6N), bl (3M))"""
    T = np.asarray(T, np.float64); X = np.asarray(X, np.float64)
    N, M = len(T), len(X)
    Hpp, bp = _edge_system(T, p)
    W = np.zeros((6 * N, 3 * M)); V = np.zeros((M, 3, 3)); bl = np.zeros((M, 3))
    bp = bp.copy()
    if oact.any():
        e, A, P = residuals(T, X, p, jac=True)
        e, A, P = e[oact], A[oact], P[oact]
        kf, lm = p["kf"][oact], p["lm"][oact]
        w = huber((e * e).sum(-1), p["huber"])[1]
        Jp = A @ np.concatenate([np.broadcast_to(np.eye(3), A.shape), -PG.hat(P)], -1)     # (O, 3, 6)
        Jl = A @ PG.rotmat(T[kf])
        wJp, wJl, we = Jp * w[:, None, None], Jl * w[:, None, None], e * w[:, None]
        r6, r3 = np.arange(6), np.arange(3)
        np.add.at(Hpp, ((kf[:, None, None] * 6 + r6[None, :, None]), (kf[:, None, None] * 6 + r6[None, None, :])), np.einsum("oij,oik->ojk", Jp, wJp))
        np.add.at(W, ((kf[:, None, None] * 6 + r6[None, :, None]), (lm[:, None, None] * 3 + r3[None, None, :])), np.einsum("oij,oik->ojk", Jp, wJl))
        np.add.at(V, lm, np.einsum("oij,oik->ojk", Jl, wJl))
        np.add.at(bp.reshape(N, 6), kf, -np.einsum("oij,oi->oj", Jp, we))
        np.add.at(bl, lm, -np.einsum("oij,oi->oj", Jl, we))
    return dict(Hpp=Hpp, W=W, V=V, bp=bp, bl=bl.reshape(-1), N=N, M=M)


def _damped_landmarks(V, lam, seen):
    """(V'^-1 with zeros at the held landmarks, free mask, whether a seen landmark's block was not positive definite)"""
    Vd = V.copy()
    i3 = np.arange(3)
    Vd[:, i3, i3] *= 1.0 + lam
    a, b, c, d, e, f = Vd[:, 0, 0], Vd[:, 0, 1], Vd[:, 0, 2], Vd[:, 1, 1], Vd[:, 1, 2], Vd[:, 2, 2]
    det = a * (d * f - e * e) + b * (c * e - b * f) + c * (b * e - c * d)
    with np.errstate(all="ignore"):
        pd = seen & (a > 0) & (a * d - b * b > 0) & (det > 0) & np.isfinite(det)
    Vi = np.zeros_like(Vd)
    if pd.any():
        Vi[pd] = np.linalg.inv(Vd[pd])
    return Vi, pd, bool((seen & ~pd).any())


def reduced_system(sysm, lam, free_kf, seen):
    """(S, b_red over the free keyframes' dofs, V'^-1, free landmarks, singular flag, dof index)"""
    N, M = sysm["N"], sysm["M"]
    dof = (np.nonzero(free_kf)[0][:, None] * 6 + np.arange(6)).ravel()
    Vi, lfree, sing = _damped_landmarks(sysm["V"], lam, seen)
    H = sysm["Hpp"][np.ix_(dof, dof)]
    H = H + lam * np.diag(np.diag(H))
    W = sysm["W"][dof]
    WV = np.einsum("amj,mjk->amk", W.reshape(len(dof), M, 3), Vi).reshape(len(dof), 3 * M)
    return H - WV @ W.T, sysm["bp"][dof] - WV @ sysm["bl"], Vi, lfree, sing, dof


def schur_step(sysm, lam, free_kf, seen, mode="dense", pcg_tol=1e-10, pcg_max_iters=4000):
    """(delta poses (N, 6), delta points (M, 3), PCG iterations, status bits)"""
    N, M = sysm["N"], sysm["M"]
    S, b, Vi, lfree, sing, dof = reduced_system(sysm, lam, free_kf, seen)
    status = FBA_SINGULAR if sing else 0
    x = np.zeros(6 * N); n_it = 0
    if len(dof):
        blocks = S.reshape(len(dof) // 6, 6, len(dof) // 6, 6)[np.arange(len(dof) // 6), :, np.arange(len(dof) // 6), :]
        if not (np.linalg.eigvalsh(blocks).min() > 0):   # (a diagonal block of S that is not positive definite: the library reports it too)
            status |= FBA_SINGULAR
        if mode == "dense":
            x[dof] = np.linalg.solve(S, b) if np.abs(b).max() > 0 else 0.0
        else:
            x[dof], n_it = PG._pcg(S, b, np.nonzero(free_kf)[0], 0, pcg_tol, pcg_max_iters)
            if n_it >= pcg_max_iters:
                status |= FBA_PCG_CAP
    dX = np.einsum("mij,mj->mi", Vi, (sysm["bl"] - sysm["W"].T @ x).reshape(M, 3))
    return x.reshape(N, 6), dX, n_it, status


def full_step(sysm, lam, free_kf, seen):
    """the same step from the undivided system [[Hpp, W], [W', V]] + lambda diag, solved densely"""
    N, M = sysm["N"], sysm["M"]
    _, lfree, _ = _damped_landmarks(sysm["V"], lam, seen)
    dof_p = (np.nonzero(free_kf)[0][:, None] * 6 + np.arange(6)).ravel()
    dof_l = (np.nonzero(lfree)[0][:, None] * 3 + np.arange(3)).ravel()
    Vfull = np.zeros((3 * M, 3 * M))
    for l in np.nonzero(lfree)[0]:
        Vfull[3 * l:3 * l + 3, 3 * l:3 * l + 3] = sysm["V"][l]
    H = np.block([[sysm["Hpp"][np.ix_(dof_p, dof_p)], sysm["W"][np.ix_(dof_p, dof_l)]], [sysm["W"][np.ix_(dof_p, dof_l)].T, Vfull[np.ix_(dof_l, dof_l)]]])
    b = np.concatenate([sysm["bp"][dof_p], sysm["bl"][dof_l]])
    sol = np.linalg.solve(H + lam * np.diag(np.diag(H)), b)
    x = np.zeros(6 * N); dX = np.zeros(3 * M)
    x[dof_p] = sol[:len(dof_p)]; dX[dof_l] = sol[len(dof_p):]
    return x.reshape(N, 6), dX.reshape(M, 3)


def apply(T, X, x, dX, free_kf):
    Tn = np.array(T, np.float64); Xn = np.asarray(X, np.float64) + dX
    if free_kf.any():
        Tn[free_kf] = PG.mul(PG.exp(x[free_kf]), Tn[free_kf])
    return Tn, Xn


def solve(p, mode="dense", polish=0, **params):
    """Levenberg-Marquardt as the module docstring states it.  Returns dict(T, X, chi2_init, chi2_final, lam, lm_iters, pcg_iters, n_free,
    n_obs_dropped, status, obs_chi2).  polish: up to that many undamped Gauss-Newton steps afterwards, each kept when the gradient norm falls (for the
    yardstick's converged state only: the library has no such phase; see tests/pose_graph_ref.py solve())."""
    P = dict(DEFAULTS); P.update(params)
    T = np.array(p["T"], np.float64).reshape(-1, 7); X = np.array(p["X"], np.float64).reshape(-1, 3)
    oact, n_drop = input_active(p)
    held = held_keyframes(p, oact); free_kf = ~held
    seen = np.zeros(len(X), bool); seen[p["lm"][oact]] = True
    c = cost(T, X, p, oact)
    out = dict(chi2_init=c, lm_iters=0, pcg_iters=0, n_free=int(free_kf.sum()), n_obs_dropped=n_drop, status=FBA_DROPPED if n_drop else 0)
    lam, fresh = P["lambda_init"], True
    todo = free_kf.any() or seen.any()
    for it in range(P["max_iters"] if todo else 0):
        if fresh:
            sysm = system(T, X, p, oact); fresh = False
        x, dX, n_it, st = schur_step(sysm, lam, free_kf, seen, mode, P["pcg_tol"], P["pcg_max_iters"])
        out["pcg_iters"] += n_it; out["status"] |= st
        Tn, Xn = apply(T, X, x, dX, free_kf)
        c_new = cost(Tn, Xn, p, oact)
        out["lm_iters"] = it + 1
        if c_new < c:
            T, X, c, fresh, lam = Tn, Xn, c_new, True, max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        if not np.sqrt((x * x).sum() + (dX * dX).sum()) >= P["step_tol"]:
            break
        if lam > 1e12:
            out["status"] |= FBA_LAMBDA
            break
    gnorm = lambda T_, X_: np.sqrt(sum((g * g).sum() for g in cost_and_gradient(T_, X_, p, oact)[1:]))
    for _ in range(polish if todo else 0):
        try:
            x, dX, _, _ = schur_step(system(T, X, p, oact), 0.0, free_kf, seen)
        except np.linalg.LinAlgError:
            break
        Tn, Xn = apply(T, X, x, dX, free_kf)
        if not (np.isfinite(cost(Tn, Xn, p, oact)) and gnorm(Tn, Xn) < gnorm(T, X)):
            break
        T, X = Tn, Xn
    if polish and todo:
        c = cost(T, X, p, oact)
    out.update(T=T, X=X, chi2_final=c, lam=lam, obs_chi2=obs_chi2(T, X, p) if len(p["kf"]) else np.zeros(0))
    return out
