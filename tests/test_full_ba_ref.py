"""CPU: guards of the full bundle adjustment yardstick (tests/full_ba_ref.py) and the argument refusals of the new entries, which need no GPU.

The GPU tests (tests/test_gpu_full_ba.py) hold the device to: poses and points within rtol 1e-4 / atol 1e-6 of the yardstick's converged state, the
exact gradient at the device's state at most 1e-6 of the initial one.  Here the yardstick itself is held to a tenth of that on every parity case (the
CASE GUARD): its own PCG mode at the library's default parameters against its converged dense mode, and two converged runs from differently perturbed
starts.  A case that fails it is not a case: tests/full_ba_cases.py says which cases were changed for that reason and how."""
import ctypes as C

import numpy as np
import pytest

import full_ba_cases as Cs
import full_ba_ref as R
import pose_graph_ref as PG


def _within_a_tenth(got, ref):
    return bool(np.all(np.abs(got["T"] - ref["T"]) <= 0.1 * (1e-6 + 1e-4 * np.abs(ref["T"]))) and
                np.all(np.abs(got["X"] - ref["X"]) <= 0.1 * (1e-6 + 1e-4 * np.abs(ref["X"]))))


def _central_differences(p, h=1e-6):
    N, M = len(p["T"]), len(p["X"])
    oact = R.input_active(p)[0]
    gT = np.zeros((N, 6)); gX = np.zeros((M, 3))
    for n in range(N):
        for k in range(6):
            d = np.zeros(6); d[k] = h
            Tp = p["T"].copy(); Tp[n] = PG.mul(PG.exp(d), Tp[n])
            Tm = p["T"].copy(); Tm[n] = PG.mul(PG.exp(-d), Tm[n])
            gT[n, k] = (R.cost(Tp, p["X"], p, oact) - R.cost(Tm, p["X"], p, oact)) / (4 * h)
    for l in range(M):
        for k in range(3):
            Xp = p["X"].copy(); Xp[l, k] += h
            Xm = p["X"].copy(); Xm[l, k] -= h
            gX[l, k] = (R.cost(p["T"], Xp, p, oact) - R.cost(p["T"], Xm, p, oact)) / (4 * h)
    return gT, gX


@pytest.mark.parametrize("case", ["plain", "huber", "edges"])
def test_gradient_matches_central_differences(case):
    """g = sum J' rho' e is the gradient of cost / 2.  The projection rows, the disparity row and the Huber branch are exact derivatives (rho' J'e is the
    gradient of rho / 2); central differences at h = 1e-6 leave h^2 times the third derivative (pixels per metre cubed: below 1e-8 of a gradient of
    1e3 - 1e5) and cost rounding 1e-16 x 1e4 / 1e-6 = 1e-6 absolute.  The edge rows carry the pose graph's series error of |r|^4 / 720.  Bound: 1e-6
    of the largest component."""
    if case == "plain":
        p = Cs.arc(4, 12, seed=2)
        assert R.stereo_mask(p).any() and not R.stereo_mask(p).all()
    elif case == "huber":
        p = Cs.arc(4, 12, seed=2, outliers=0.2, huber=np.sqrt(5.991))
        s = R.obs_chi2(p["T"], p["X"], p)
        assert (s > 5.991).any() and (s < 5.991).any()   # both branches
    else:
        p = Cs.ring(N=24, M=60, L=1)
    _, gT, gX = R.cost_and_gradient(p["T"], p["X"], p)
    nT, nX = _central_differences(p)
    held = R.held_keyframes(p)
    nT[held] = 0
    top = max(np.abs(gT).max(), np.abs(gX).max())
    print("%s: largest component %.3e, largest difference %.3e" % (case, top, max(np.abs(nT - gT).max(), np.abs(nX - gX).max())))
    assert np.all(gT[held] == 0) and top > 1.0
    assert np.abs(nT - gT).max() <= 1e-6 * top and np.abs(nX - gX).max() <= 1e-6 * top


def test_disparity_row_is_part_of_the_gradient():
    p = Cs.arc(4, 12, seed=2)
    g1 = R.cost_and_gradient(p["T"], p["X"], p)[2]
    g0 = R.cost_and_gradient(p["T"], p["X"], Cs.without(p, disp=None))[2]
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g1).max()


@pytest.mark.parametrize("lam", [1e-4, 1.0])
def test_schur_solve_equals_the_full_dense_solve(lam):
    for p in (Cs.arc(12, 63), Cs.ring(N=24, M=80, L=2), Cs.huber_case()):
        oact = R.input_active(p)[0]
        free = ~R.held_keyframes(p, oact)
        seen = np.zeros(len(p["X"]), bool); seen[p["lm"][oact]] = True
        sysm = R.system(p["T"], p["X"], p, oact)
        x, dX, _, st = R.schur_step(sysm, lam, free, seen)
        xf, dXf = R.full_step(sysm, lam, free, seen)
        scale = max(np.abs(xf).max(), np.abs(dXf).max())
        assert st == 0 and scale > 1e-4
        assert np.abs(x - xf).max() <= 1e-8 * scale and np.abs(dX - dXf).max() <= 1e-8 * scale


def test_schur_gradient_is_cost_and_gradient():
    """the right-hand sides system() builds are minus the gradient cost_and_gradient() walks"""
    p = Cs.ring(N=24, M=80, L=2)
    oact = R.input_active(p)[0]
    sysm = R.system(p["T"], p["X"], p, oact)
    _, gT, gX = R.cost_and_gradient(p["T"], p["X"], p)
    free = ~R.held_keyframes(p)
    assert np.allclose(-sysm["bp"].reshape(-1, 6)[free], gT[free], rtol=1e-12, atol=1e-9) and np.allclose(-sysm["bl"].reshape(-1, 3), gX, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("name", Cs.PARITY_NAMES)
def test_case_guard(name):
    """every parity case, the yardstick alone: PCG at the library's defaults against the converged dense state, and a second converged run from another
    start, within one tenth of the GPU parity tolerance; the gradient at a tenth of the GPU bound"""
    p, ref = Cs.reference(name)
    two = R.solve(Cs.perturbed(p, seed=7), **Cs.CONVERGED)
    pcg = R.solve(p, mode="pcg")
    g0 = Cs.gradient_norm(p, p["T"], p["X"])
    gn = Cs.gradient_norm(p, pcg["T"], pcg["X"])
    print("%s: %d keyframes %d landmarks %d observations; two starts %.2e apart; pcg mode %.2e from converged, gradient %.2e of initial, %d LM / %d PCG iterations"
          % (name, len(p["T"]), len(p["X"]), len(p["kf"]), max(np.abs(two["T"] - ref["T"]).max(), np.abs(two["X"] - ref["X"]).max()),
             max(np.abs(pcg["T"] - ref["T"]).max(), np.abs(pcg["X"] - ref["X"]).max()), gn / g0, pcg["lm_iters"], pcg["pcg_iters"]))
    assert _within_a_tenth(two, ref)
    assert _within_a_tenth(pcg, ref)
    assert gn <= 1e-7 * g0 and pcg["status"] == 0 and ref["status"] == 0
    assert pcg["chi2_final"] < pcg["chi2_init"]
    assert pcg["pcg_iters"] < R.DEFAULTS["pcg_max_iters"]


def test_the_inputs_matter():
    """the guards the GPU parity test leans on: Huber, the loop edges and the disparities each move the answer by more than the parity tolerance"""
    far = lambda a, b: not (np.allclose(a["T"], b["T"], rtol=1e-4, atol=1e-6) and np.allclose(a["X"], b["X"], rtol=1e-4, atol=1e-6))
    p, ref = Cs.reference("huber")
    assert far(R.solve(Cs.without(p, huber=0.0), **Cs.CONVERGED), ref)
    p, ref = Cs.reference("ring_5")
    assert far(R.solve(Cs.no_edges(p), **Cs.CONVERGED), ref)
    p, ref = Cs.reference("arc_12_63")
    assert far(R.solve(Cs.without(p, disp=None), **Cs.CONVERGED), ref)


def test_degenerate_problems_are_results():
    for name, (p, n_free, status, dropped) in Cs.degenerate().items():
        r = R.solve(p)
        assert (r["n_free"], r["status"], r["n_obs_dropped"]) == (n_free, status, dropped), (name, r["n_free"], r["status"], r["n_obs_dropped"])
        assert np.isfinite(r["T"]).all() and np.isfinite(r["X"]).all() and np.isfinite(r["chi2_final"]) and r["chi2_final"] <= r["chi2_init"], name
        if n_free == 0:
            assert np.array_equal(r["T"], p["T"]), name


def test_pack_lays_problems_back_to_back():
    ps = [Cs.arc(2, 63), Cs.ring(N=24, M=80, L=2), Cs.arc(12, 1)]
    b = Cs.pack(ps)
    assert list(b["kf_off"]) == [0, 2, 26, 38] and b["obs_off"][-1] == sum(len(p["kf"]) for p in ps) and list(b["edge_off"]) == [0, 0, 2, 2]
    assert b["fixed"] is not None and list(b["fixed"][:3]) == [1, 0, 1] and b["fixed"][26:].all()
    assert (np.diff(b["lm"][b["obs_off"][1]:b["obs_off"][2]]) >= 0).all()


# ------------------------------------------------------------------------------------------ argument refusals: no GPU needed
def test_default_params_and_struct_sizes(pkg):
    p = pkg.default_full_ba_params()
    assert p.struct_size == C.sizeof(pkg.FullBAParams) == 40
    assert (p.max_iters, p.pcg_max_iters, p.pcg_tol, p.step_tol, p.lambda_init) == tuple(R.DEFAULTS[k] for k in ("max_iters", "pcg_max_iters", "pcg_tol", "step_tol", "lambda_init"))
    assert C.sizeof(pkg.FullBABatch) == 24 + 18 * 8 + 6 * 8 and pkg.FULL_BA_STATS_DTYPE.itemsize == 48
    assert (pkg.FBA_BAD_INDEX, pkg.FBA_NONFINITE, pkg.FBA_PCG_CAP, pkg.FBA_LAMBDA, pkg.FBA_SINGULAR, pkg.FBA_DROPPED) == \
        (R.FBA_BAD_INDEX, R.FBA_NONFINITE, R.FBA_PCG_CAP, R.FBA_LAMBDA, R.FBA_SINGULAR, R.FBA_DROPPED)


def test_full_ba_entries_refuse_bad_arguments(pkg):
    """every refusal comes with VSLAM_ERR_ARG and a message naming its cause, before a context is looked at (so a null context reaches them all)"""
    lib = pkg.load_library()
    err = lambda: lib.vslam_last_error().decode()
    one = C.c_void_p(8)   # a non-null pointer that is never dereferenced: every call below is refused on the host

    def batch(**kw):
        b = pkg.FullBABatch(struct_size=C.sizeof(pkg.FullBABatch), n_problems=1, total_kfs=2, total_lms=1, total_obs=2, total_edges=1, d_kf_off=one, d_lm_off=one,
                            d_obs_off=one, d_edge_off=one, d_T=one, d_xyz=one, d_obs_kf=one, d_obs_lm=one, d_obs_uv=one, d_edge_i=one, d_edge_j=one, d_edge_Z=one,
                            d_edge_w=one, K4=(C.c_double * 4)(700.0, 700.0, 600.0, 180.0), bf=400.0, huber_delta=0.0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(b, p=None, T_out=one, X_out=one):
        return lib.vslam_full_ba_dev(None, C.byref(b) if b is not None else None, C.byref(p) if p is not None else None, T_out, X_out, None)

    assert call(None) == pkg.VSLAM_ERR_ARG and "null problem" in err()
    assert call(batch(struct_size=0)) == pkg.VSLAM_ERR_ARG and "struct_size" in err()
    assert call(batch(struct_size=C.sizeof(pkg.FullBABatch) + 8)) == pkg.VSLAM_ERR_ARG and "struct_size" in err()
    assert call(batch(), pkg.default_full_ba_params(struct_size=4)) == pkg.VSLAM_ERR_ARG and "vslam_full_ba_params struct_size" in err()
    for field in ("n_problems", "total_kfs", "total_lms", "total_obs", "total_edges"):
        assert call(batch(**{field: -1})) == pkg.VSLAM_ERR_ARG and "negative count" in err(), field
    for field in ("d_kf_off", "d_lm_off", "d_obs_off", "d_edge_off", "d_T", "d_xyz", "d_obs_kf", "d_obs_lm", "d_obs_uv", "d_edge_i", "d_edge_j", "d_edge_Z", "d_edge_w"):
        assert call(batch(**{field: None})) == pkg.VSLAM_ERR_ARG and "null d_" in err(), field
    assert call(batch(), T_out=None) == pkg.VSLAM_ERR_ARG and "d_T_out" in err()
    assert call(batch(), X_out=None) == pkg.VSLAM_ERR_ARG and "d_xyz_out" in err()
    for kw in (dict(max_iters=-1), dict(pcg_max_iters=0), dict(pcg_tol=-1.0), dict(step_tol=float("nan")), dict(lambda_init=0.0)):
        assert call(batch(), pkg.default_full_ba_params(**kw)) == pkg.VSLAM_ERR_ARG and "parameters out of range" in err(), kw
    for kw in (dict(K4=(C.c_double * 4)(0.0, 700.0, 600.0, 180.0)), dict(K4=(C.c_double * 4)(700.0, 700.0, float("nan"), 180.0)), dict(bf=-1.0), dict(bf=float("inf")),
               dict(huber_delta=-1.0), dict(huber_delta=float("nan"))):
        assert call(batch(**kw)) == pkg.VSLAM_ERR_ARG and "camera out of range" in err(), kw
    # the optional pointers may be null, and so may the edge arrays when there are no edges
    assert call(batch(total_edges=0, d_edge_i=None, d_edge_j=None, d_edge_Z=None, d_edge_w=None)) == pkg.VSLAM_ERR_ARG and "null context" in err()
    assert call(batch()) == pkg.VSLAM_ERR_ARG and "null context" in err()
    st = np.zeros(1, np.int32)
    assert lib.vslam_full_ba_status_dev(None, 1, None) == pkg.VSLAM_ERR_ARG and "null h_status" in err()
    assert lib.vslam_full_ba_status_dev(None, -1, st) == pkg.VSLAM_ERR_ARG and "negative" in err()
    assert lib.vslam_full_ba_status_dev(None, 1, st) == pkg.VSLAM_ERR_ARG and "null context" in err()


def test_fba_store_is_a_tuning_key():
    import stereo_visual_slam_amd as pkg
    blob = open(pkg._SO, "rb").read()
    assert b"fba_store" in blob and b"VSLAM_FBA_STORE" in blob
