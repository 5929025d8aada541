"""Seeded full bundle adjustment problems (the dicts tests/full_ba_ref.py takes): a camera on an arc with the project's default intrinsics, landmarks
6 - 35 m ahead of the last keyframe that sees them, each seen by a run of consecutive keyframes, the creating observation stereo (and three in ten of
the others, so that valid and NaN disparities mix), 0.3 px of noise on pixels and disparities, initial poses and points perturbed.  pack() lays
several problems back to back.

Sizes.  N in {2, 12, 65} keyframes, M in {1, 63, 64, 65, 300} landmarks: one landmark, the two sides of a 64-index block, several blocks.  Two
departures from "3 - 8 keyframes per landmark", each forced by the case guard of tests/test_full_ba_ref.py (the minimum must be unique):
  * M = 1: one landmark gives at most 3 rows per keyframe against 6 unknowns, so no pose is determined; every keyframe is held and the problem is
    the triangulation of the landmark.
  * N = 65 with M <= 65: at 3 - 8 keyframes per landmark a keyframe would see five landmarks on average and some fewer than three; the run length
    is raised until a keyframe sees twelve on average (RUN_TARGET).
TRIMMED cases cut a problem to an exact observation count on both sides of 256 (the kernel's workgroup width: where a lane-strided loop takes its
second trip) and of 512 (its third).
input_cases() varies what a problem may say besides its size: held keyframes, the observation mask, and the mask, weights and direction of edges."""
import functools

import numpy as np

import full_ba_ref as R
import pose_graph_ref as PG

K4 = (718.856, 718.856, 607.1928, 185.2157)
BF = 718.856 * 0.573
SIZES = [(N, M) for N in (2, 12, 65) for M in (1, 63, 64, 65, 300)]
TRIMMED = [(12, 64, 255), (12, 64, 256), (12, 64, 257), (12, 110, 511), (12, 110, 512), (12, 110, 513)]
RUN_TARGET = 12
CONVERGED = R.CONVERGED


def _arc_poses(N, step=0.5, rad=40.0, lap=False):
    """T_c_w of a camera that drives along a circle in the x-z plane, looking along the tangent (z forward at keyframe 0)"""
    a = 2 * np.pi * np.arange(N) / N if lap else step * np.arange(N) / rad
    if lap:
        rad = step * N / (2 * np.pi)
    Twc = np.zeros((N, 7))
    Twc[:, 1] = np.sin(-a / 2); Twc[:, 3] = np.cos(-a / 2)
    Twc[:, 4] = -rad * (1 - np.cos(a)); Twc[:, 5] = 0.02 * np.sin(5 * a); Twc[:, 6] = rad * np.sin(a)
    return PG.inverse(Twc)


def _observe(Tt, first, last, rng, lateral=0.35, stereo_extra=0.3, noise=0.3, depth=(6.0, 35.0)):
    """landmarks in front of their last observer, and their observations sorted by landmark"""
    M = len(first)
    z = rng.uniform(depth[0], depth[1], M)
    Pl = np.stack([rng.uniform(-lateral, lateral, M) * z, rng.uniform(-0.12, 0.12, M) * z, z], -1)
    Tl = PG.inverse(Tt[last])
    X = np.einsum("mij,mj->mi", PG.rotmat(Tl), Pl) + Tl[:, 4:]
    kf = np.concatenate([np.arange(first[l], last[l] + 1) for l in range(M)]).astype(np.int32)
    lm = np.concatenate([np.full(last[l] - first[l] + 1, l) for l in range(M)]).astype(np.int32)
    P = np.einsum("oij,oj->oi", PG.rotmat(Tt[kf]), X[lm]) + Tt[kf, 4:]
    assert (P[:, 2] > 1.0).all()
    uv = np.stack([K4[0] * P[:, 0] / P[:, 2] + K4[2], K4[1] * P[:, 1] / P[:, 2] + K4[3]], -1) + rng.normal(0, noise, (len(kf), 2))
    disp = BF / P[:, 2] + rng.normal(0, noise, len(kf))
    creating = np.concatenate([[True], lm[1:] != lm[:-1]])
    stereo = creating | (rng.random(len(kf)) < stereo_extra)
    disp = np.where(stereo, np.maximum(disp, 0.0), np.where(rng.random(len(kf)) < 0.5, np.nan, -1.0))
    return X, kf, lm, uv.astype(np.float32), disp.astype(np.float32)


def _empty_edges():
    return dict(ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), Z=np.zeros((0, 7)), w=np.zeros((0, 6)), edge_active=None)


def arc(N, M, seed=0, trim_to=None, outliers=0.0, huber=0.0, s_pose=(0.03, 0.006), s_point=0.05, run=None, depth=(6.0, 35.0)):
    rng = np.random.default_rng(100000 * N + 10 * M + seed)
    Tt = _arc_poses(N)
    lo = min(N, max(3, -(-RUN_TARGET * N // max(M, 1)))) if M > 1 else min(N, 8)
    hi = min(N, max(8, lo + 5)) if M > 1 else lo
    lo, hi = (lo, hi) if run is None else run
    run = rng.integers(lo, hi + 1, M)
    # track centres spread evenly over the arc; tracks that would stick out are pushed back in, so the first and last keyframes see the most
    first = np.clip(np.round(np.linspace(0, N - 1, M) if M > 1 else np.zeros(1)).astype(np.int64) - run // 2, 0, N - run)
    X, kf, lm, uv, disp = _observe(Tt, first, first + run - 1, rng, depth=depth)
    if trim_to is not None:   # until the count is exact: the keyframe with the most observations loses one, of its longest track, never a creating one
        keep = np.ones(len(kf), bool)
        creating = np.concatenate([[True], lm[1:] != lm[:-1]])
        while keep.sum() > trim_to:
            cnt = np.bincount(lm[keep], minlength=M)
            k = int(np.argmax(np.bincount(kf[keep], minlength=N)))
            cand = np.nonzero(keep & (kf == k) & ~creating & (cnt[lm] > 3))[0]
            keep[cand[np.argmax(cnt[lm[cand]])]] = False
        kf, lm, uv, disp = kf[keep], lm[keep], uv[keep], disp[keep]
    if outliers > 0:
        bad = rng.choice(len(kf), max(1, int(round(outliers * len(kf)))), replace=False)
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        uv = uv.copy(); uv[bad] += (50.0 * np.stack([np.cos(ang), np.sin(ang)], -1)).astype(np.float32)
    T0 = Tt.copy()
    fixed = None
    if M == 1:
        fixed = np.ones(N, np.uint8)
    else:
        T0[1:] = PG.mul(PG.exp(np.concatenate([rng.normal(0, s_pose[0], (N - 1, 3)), rng.normal(0, s_pose[1], (N - 1, 3))], -1)), Tt[1:])
    X0 = X + rng.normal(0, s_point, X.shape)
    return dict(_empty_edges(), T=T0, X=X0, kf=kf, lm=lm, uv=uv, disp=disp, fixed=fixed, obs_active=None, K4=K4, bf=BF, huber=float(huber), T_true=Tt, X_true=X)


def huber_case():
    """5 % of the observations displaced by 50 px; width sqrt(5.991), the library's.  Gauss-Newton on Huber weights converges linearly, at a rate set
    by how much of a landmark's information sits in its outliers: at 3 - 8 observations per landmark 6 - 35 m away a four-observation landmark with
    one outlier was still moving by 5e-4 after 100 iterations, so this case has 6 - 8 observations per landmark, 6 - 20 m away."""
    return arc(12, 120, seed=5, outliers=0.05, huber=np.sqrt(5.991), run=(6, 8), depth=(6.0, 20.0))


def ring(N=40, M=260, L=1, seed=0, w_loop=(400.0, 4000.0)):
    """One lap (2 m per keyframe).  The initial poses chain noisy odometry from keyframe 0 and so drift; a landmark is seen by 3 - 5 consecutive
    keyframes, none across the seam between the last keyframe and the first, so only the L loop edges (late keyframe q against early keyframe c) tie
    the end of the lap to its start.  Initial points: the true point carried by its creating keyframe's drift."""
    rng = np.random.default_rng(7000 * N + 10 * L + seed)
    Tt = _arc_poses(N, step=2.0, lap=True)
    run = rng.integers(3, 6, M)
    first = np.clip(np.floor(np.linspace(0, 1, M, endpoint=False) * (N - run + 1)).astype(np.int64), 0, N - run)
    X, kf, lm, uv, disp = _observe(Tt, first, first + run - 1, rng, lateral=0.15)
    noise = lambda n, s_t, s_r: PG.exp(np.concatenate([rng.normal(0, s_t, (n, 3)), rng.normal(0, s_r, (n, 3))], -1))
    Zo = PG.mul(noise(N - 1, 0.01, 0.002), PG.mul(Tt[1:], PG.inverse(Tt[:-1])))
    T0 = np.zeros((N, 7)); T0[0] = Tt[0]
    for k in range(1, N):
        T0[k] = PG.mul(Zo[k - 1], T0[k - 1])
    lq = N - 1 - np.arange(L) * 2; lc = np.arange(L) * 3
    Zl = PG.mul(noise(L, 0.01, 0.001), PG.mul(Tt[lq], PG.inverse(Tt[lc])))
    corr = PG.mul(PG.inverse(T0[first]), Tt[first])   # X0 = T0^-1 Tt X
    X0 = np.einsum("mij,mj->mi", PG.rotmat(corr), X) + corr[:, 4:]
    return dict(T=T0, X=X0, kf=kf, lm=lm, uv=uv, disp=disp, fixed=None, obs_active=None, K4=K4, bf=BF, huber=0.0, ei=lq.astype(np.int32), ej=lc.astype(np.int32),
                Z=Zl, w=np.tile(np.repeat(np.asarray(w_loop, np.float64), 3), (L, 1)), edge_active=None, T_true=Tt, X_true=X)


def perturbed(p, seed, s_pose=(0.02, 0.004), s_point=0.03):
    """the second start of the case guard: every free pose and every point moved"""
    rng = np.random.default_rng(seed)
    T = p["T"].copy(); X = p["X"] + rng.normal(0, s_point, p["X"].shape)
    free = ~R.held_keyframes(p)
    n = int(free.sum())
    if n:
        T[free] = PG.mul(PG.exp(np.concatenate([rng.normal(0, s_pose[0], (n, 3)), rng.normal(0, s_pose[1], (n, 3))], -1)), T[free])
    return dict(p, T=T, X=X)


def without(p, **kw):
    """a copy with fields replaced (disp=None: no disparities; ei ... empty: no edges)"""
    q = dict(p); q.update(kw)
    return q


def no_edges(p):
    return without(p, **_empty_edges())


def degenerate():
    """{name: (problem, expected n_free, expected status, expected n_obs_dropped)}: every one is a result with finite output"""
    base = arc(12, 63, seed=3)
    cut = lambda keep: dict(base, kf=base["kf"][keep], lm=base["lm"][keep], uv=base["uv"][keep], disp=base["disp"][keep])
    none = np.zeros(len(base["kf"]), bool)
    out = {}
    out["no_observations"] = (cut(none), 0, 0, 0)
    one = dict(base, T=base["T"][:1].copy())
    k0 = base["kf"] == 0
    out["one_keyframe"] = (dict(one, kf=base["kf"][k0], lm=base["lm"][k0], uv=base["uv"][k0], disp=base["disp"][k0]), 0, 0, 0)
    out["all_held"] = (dict(base, fixed=np.ones(12, np.uint8)), 0, 0, 0)
    out["keyframe_without_observations"] = (cut(base["kf"] != 5), 10, 0, 0)
    # one extra landmark seen once: with a disparity it is a stereo triangulation (3 rows, 3 unknowns), without it has 2 rows and moves under
    # damping alone along its ray
    for name, d in (("single_stereo_landmark", 20.0), ("single_mono_landmark", np.nan)):
        X = np.concatenate([base["X"], [[0.5, 0.2, 20.0]]])
        out[name] = (dict(base, X=X, kf=np.append(base["kf"], 0).astype(np.int32), lm=np.append(base["lm"], 63).astype(np.int32),
                          uv=np.concatenate([base["uv"], [[620.0, 190.0]]]).astype(np.float32), disp=np.append(base["disp"], d).astype(np.float32)), 11, 0, 0)
    # landmark 7 put behind its observers at the input: all its observations are dropped for the call
    X = base["X"].copy(); o7 = np.nonzero(base["lm"] == 7)[0]
    Tk = PG.inverse(base["T"][base["kf"][o7[0]]])
    X[7] = PG.rotmat(Tk) @ np.array([0.3, 0.1, -4.0]) + Tk[4:]
    out["observation_behind_camera"] = (dict(base, X=X), 11, R.FBA_DROPPED, len(o7))
    # no observations and edges that weigh nothing: H = 0
    e = dict(ei=np.arange(1, 12).astype(np.int32), ej=np.arange(0, 11).astype(np.int32), Z=PG.mul(base["T"][1:], PG.inverse(base["T"][:-1])), w=np.zeros((11, 6)))
    out["all_weights_zero"] = (dict(cut(none), **e), 11, R.FBA_SINGULAR, 0)
    return out


def pack(problems):
    """dict(T, X, kf_off, lm_off, obs_off, edge_off, kf, lm, uv, disp or None, ei, ej, Z, w, fixed or None, obs_active or None, edge_active or None)"""
    off = lambda k: np.cumsum([0] + [len(p[k]) for p in problems]).astype(np.int32)
    cat = lambda k, shape, dt: np.concatenate([np.asarray(p[k], dt).reshape(shape) for p in problems]) if problems else np.zeros(shape, dt).reshape(shape)
    out = dict(kf_off=off("T"), lm_off=off("X"), obs_off=off("kf"), edge_off=off("ei"), T=cat("T", (-1, 7), np.float64), X=cat("X", (-1, 3), np.float64),
               kf=cat("kf", (-1,), np.int32), lm=cat("lm", (-1,), np.int32), uv=cat("uv", (-1, 2), np.float32), ei=cat("ei", (-1,), np.int32),
               ej=cat("ej", (-1,), np.int32), Z=cat("Z", (-1, 7), np.float64), w=cat("w", (-1, 6), np.float64), disp=None, fixed=None, obs_active=None, edge_active=None)
    if any(p.get("disp") is not None for p in problems):
        out["disp"] = np.concatenate([np.asarray(p["disp"], np.float32) if p.get("disp") is not None else np.full(len(p["kf"]), -1.0, np.float32) for p in problems])
    if any(p.get("fixed") is not None for p in problems):
        out["fixed"] = np.concatenate([np.asarray(p["fixed"], np.uint8) if p.get("fixed") is not None else (np.arange(len(p["T"])) == 0).astype(np.uint8) for p in problems])
    for key, n in (("obs_active", "kf"), ("edge_active", "ei")):
        if any(p.get(key) is not None for p in problems):
            out[key] = np.concatenate([np.asarray(p[key], np.uint8) if p.get(key) is not None else np.ones(len(p[n]), np.uint8) for p in problems])
    return out


@functools.lru_cache(maxsize=None)
def parity_cases():
    """{name: problem} of every case the GPU parity test runs and the CPU case guard vouches for"""
    cases = {"arc_%d_%d" % (N, M): arc(N, M) for N, M in SIZES}
    cases.update({"arc_%d_%d_obs%d" % (N, M, O): arc(N, M, seed=1, trim_to=O) for N, M, O in TRIMMED})
    cases["huber"] = huber_case()
    cases["ring_1"] = ring(L=1); cases["ring_5"] = ring(L=5)
    return cases


PARITY_NAMES = ["arc_%d_%d" % s for s in SIZES] + ["arc_%d_%d_obs%d" % t for t in TRIMMED] + ["huber", "ring_1", "ring_5"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem, the yardstick's converged result): computed once, shared by the CPU guard and the GPU tests, never modified"""
    p = parity_cases()[name]
    ref = R.solve(p, **CONVERGED)
    for v in list(p.values()) + [ref["T"], ref["X"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p, ref


# ------------------------------------------------------------------------------------------ the input space: masks, held keyframes, edge weights, directions
OBS_MASK = dict(kf_off=5, lm_off=20, lm_behind=7)


def _obs_mask_case():
    """arc(12, 63) under an observation mask: keyframe kf_off and landmark lm_off have every observation off (both are then held / copied through);
    holes at the first, a middle and the last position of other landmarks' ranges, four of each, taken only where the landmark keeps three active
    observations of which one is stereo (a landmark left with mono views only has no unique minimum); landmark lm_behind stands behind its observers
    at the input, as in degenerate(), and one of its observations is masked off too, so that n_obs_dropped counts the others only."""
    p = arc(12, 63)
    kf, lm = p["kf"], p["lm"]
    O = len(kf)
    stereo = R.stereo_mask(p)
    act = np.ones(O, bool)
    act[kf == OBS_MASK["kf_off"]] = False
    act[lm == OBS_MASK["lm_off"]] = False
    o7 = np.nonzero(lm == OBS_MASK["lm_behind"])[0]
    X = p["X"].copy()
    Tk = PG.inverse(p["T"][kf[o7[0]]])
    X[OBS_MASK["lm_behind"]] = PG.rotmat(Tk) @ np.array([0.3, 0.1, -4.0]) + Tk[4:]
    act[o7[len(o7) // 2]] = False
    holes = {"first": [], "middle": [], "last": []}
    for l in range(len(X)):
        kind = min(holes, key=lambda k: len(holes[k]))
        o = np.nonzero(lm == l)[0]
        if l in (OBS_MASK["lm_off"], OBS_MASK["lm_behind"]) or len(holes[kind]) >= 4:
            continue
        at = {"first": o[0], "middle": o[len(o) // 2], "last": o[-1]}[kind]
        rest = o[(o != at) & act[o]]
        if act[at] and len(rest) >= 3 and stereo[rest].any():
            act[at] = False
            holes[kind].append(int(at))
    assert all(len(v) == 4 for v in holes.values())
    return dict(p, X=X, obs_active=act.astype(np.uint8)), holes


def reverse_edges(p, which):
    """a copy whose edges `which` (indices) are stored the other way round, (j, i, Z^-1)"""
    ei, ej, Z = p["ei"].copy(), p["ej"].copy(), p["Z"].copy()
    ei[which], ej[which] = p["ej"][which], p["ei"][which]
    Z[which] = PG.inverse(p["Z"][which])
    return dict(p, ei=ei, ej=ej, Z=Z)


def held(N, kfs):
    f = np.zeros(N, np.uint8); f[list(kfs)] = 1
    return f


@functools.lru_cache(maxsize=None)
def input_cases():
    """{name: problem} of the cases that vary what parity_cases() leaves alone: which keyframes are held, the observation mask, and on the edges of
    ring_5 the mask, weights per edge and axis, and the direction"""
    a, r5 = arc(12, 63), ring(L=5)
    rng = np.random.default_rng(2121)
    out = {}
    out["held_01"] = dict(a, fixed=held(12, [0, 1]))
    out["held_mid"] = dict(a, fixed=held(12, [6]))          # keyframe 0 is free
    out["obs_mask"] = _obs_mask_case()[0]
    out["edge_mask"] = dict(r5, edge_active=np.array([1, 0, 1, 0, 1], np.uint8))
    out["edge_weights"] = dict(r5, w=r5["w"] * np.exp(rng.uniform(np.log(0.2), np.log(5.0), (5, 6))))
    out["edge_reversed"] = reverse_edges(r5, [0, 2])
    for p in out.values():
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


INPUT_NAMES = ["held_01", "held_mid", "obs_mask", "edge_mask", "edge_weights", "edge_reversed"]


@functools.lru_cache(maxsize=None)
def input_reference(name):
    """(problem, the yardstick's converged result): computed once, shared by the CPU guard and the GPU tests, never modified"""
    p = input_cases()[name]
    ref = R.solve(p, **CONVERGED)
    ref["T"].setflags(write=False); ref["X"].setflags(write=False)
    return p, ref


def seen_landmarks(p):
    """the landmarks with an active observation in the call: the others are copied through"""
    seen = np.zeros(len(p["X"]), bool); seen[p["lm"][R.input_active(p)[0]]] = True
    return seen


def gradient_norm(p, T, X):
    _, gT, gX = R.cost_and_gradient(T, X, p)
    return float(np.sqrt((gT * gT).sum() + (gX * gX).sum()))
