"""CPU: guards of the pose-graph yardstick (tests/pose_graph_ref.py) and the argument refusals of the new entries, which need no GPU.

The GPU tests (tests/test_gpu_pose_graph.py) hold the device to: poses within rtol 1e-4 / atol 1e-6 of the yardstick's converged poses, chi2_final at most
the yardstick's x (1 + 1e-9), the exact gradient at the device's poses at most 1e-6 of the initial one.  Here the yardstick itself is held to them with a
factor ten to spare, by its own PCG mode at the library's default parameters, and its converged poses are shown to be a property of the problem: two
starts end within 1e-9."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cases as Cs
import pose_graph_ref as R

RINGS = [(N, L) for N in Cs.RING_NODES for L in Cs.RING_LOOPS]


def test_se3_round_trips():
    rng = np.random.default_rng(0)
    xi = rng.normal(0, 0.5, (50, 6))
    T = R.exp(xi)
    assert np.allclose(R.log(T), xi, atol=1e-12)
    assert np.allclose(R.mul(T, R.inverse(T))[:, 3:], np.array([1.0, 0, 0, 0]), atol=1e-12)
    # Ad(T) xi is the tangent of T exp(xi) T^-1
    d = rng.normal(0, 1e-3, (50, 6))
    lhs = R.log(R.mul(R.mul(T, R.exp(d)), R.inverse(T)))
    assert np.allclose(lhs, np.einsum("nij,nj->ni", R.Ad(T), d), atol=1e-12)


def test_gradient_matches_central_differences():
    """g_n = sum J' W r is the gradient of cost / 2 under T <- exp(delta) T.  A is the series of the inverse left Jacobian cut after ad^2, so the analytic
    gradient is off by |r|^4 / 720 of itself (residuals here are below 0.05: 1e-8); central differences at h = 1e-6 add 1e-10 of curvature error and
    1e-16 / 1e-6 of rounding.  Bound: 1e-7 of the largest component."""
    g = Cs.ring(12, 5)
    c0, grad = R.cost_and_gradient(g["T"], g["ei"], g["ej"], g["Z"], g["w"])
    assert np.abs(R.residuals(g["T"], g["ei"], g["ej"], g["Z"])[0]).max() < 0.05
    h = 1e-6
    num = np.zeros_like(grad)
    for n in range(1, 12):
        for k in range(6):
            d = np.zeros(6); d[k] = h
            Tp = g["T"].copy(); Tp[n] = R.mul(R.exp(d), Tp[n])
            Tm = g["T"].copy(); Tm[n] = R.mul(R.exp(-d), Tm[n])
            num[n, k] = (R.cost_and_gradient(Tp, g["ei"], g["ej"], g["Z"], g["w"])[0] - R.cost_and_gradient(Tm, g["ei"], g["ej"], g["Z"], g["w"])[0]) / (4 * h)
    assert np.all(grad[0] == 0)
    assert np.abs(num - grad).max() <= 1e-7 * np.abs(grad).max()


def test_shortcut_jacobian_is_not_the_gradient():
    """why A is required: with A = I the 'gradient' differs from the central differences at the 1e-3 level on the same graph"""
    g = Cs.ring(12, 5)
    r, Em, Zi = R.residuals(g["T"], g["ei"], g["ej"], g["Z"])
    Ji, _ = R.jacobians(r, Em, Zi); Ji0, _ = R.jacobians(r, Em, Zi, exact_A=False)
    assert np.abs(Ji - Ji0).max() > 1e-3


@pytest.mark.parametrize("N,L", RINGS)
def test_two_starts_end_at_the_same_poses(N, L):
    g, ref = Cs.ring_reference(N, L)
    g2 = Cs.perturbed(g, seed=7)
    assert np.abs(g2["T"] - g["T"]).max() > 1e-3
    r2 = R.solve(g2["T"], g["ei"], g["ej"], g["Z"], g["w"], **Cs.CONVERGED)
    d = np.abs(r2["T"] - ref["T"]).max()
    print("ring %d/%d: two starts %.2e apart" % (N, L, d))
    assert d <= 1e-9


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("N,L", RINGS)
def test_pcg_mode_meets_the_gpu_bounds_with_a_factor_ten(N, L, precond):
    g, ref = Cs.ring_reference(N, L)
    r = R.solve(g["T"], g["ei"], g["ej"], g["Z"], g["w"], mode="pcg", precond=precond)
    g0 = Cs.gradient_norm(g, g["T"])
    dT = np.abs(r["T"] - ref["T"]); gn = Cs.gradient_norm(g, r["T"])
    print("ring %d/%d precond %d: dT %.2e chi2 ratio - 1 %.2e gradient %.2e of initial, %d LM / %d PCG iterations"
          % (N, L, precond, dT.max(), r["chi2_final"] / ref["chi2_final"] - 1, gn / g0, r["lm_iters"], r["pcg_iters"]))
    assert np.all(dT <= 0.1 * (1e-6 + 1e-4 * np.abs(ref["T"])))
    assert r["chi2_final"] <= ref["chi2_final"] * (1 + 1e-10)
    assert gn <= 1e-7 * g0
    assert r["chi2_final"] < r["chi2_init"]


def test_degenerate_graphs_are_results():
    for name, (g, n_free) in Cs.degenerate().items():
        r = R.solve(g["T"], g["ei"], g["ej"], g["Z"], g["w"], g["fixed"], g["active"])
        assert r["n_free"] == n_free, name
        assert np.isfinite(r["T"]).all() and np.isfinite(r["chi2_final"]) and r["chi2_final"] <= r["chi2_init"], name
        if n_free == 0:
            assert np.array_equal(r["T"], g["T"]) and r["lm_iters"] == 0, name


# ------------------------------------------------------------------------------------------ the input cases (tests/test_gpu_pose_graph_inputs.py)
def _far(T, ref_T):
    """farther than the GPU parity tolerance"""
    return not np.allclose(T, ref_T, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", Cs.INPUT_NAMES)
def test_input_case_guard(name):
    """every input case, the yardstick alone, as the rings above: two converged starts within 1e-9, its PCG mode at the library's defaults under both
    preconditioners within a tenth of the GPU parity tolerance, gradient at a tenth of the GPU bound.  Held nodes are compared with the input.
    zero_weight_node is guarded on the graph its reference is taken from (its node without edges)."""
    g, ref = Cs.input_reference(name)
    y = Cs.yardstick_graph(name)
    hold = Cs.held_of(y)
    assert ref["n_free"] == int((~hold).sum()) and np.array_equal(ref["T"][hold], g["T"][hold])
    y2 = Cs.perturbed(y, seed=7)
    assert np.abs(y2["T"] - y["T"])[~hold].max() > 1e-3 and np.array_equal(y2["T"][hold], y["T"][hold])
    two = Cs.solve_case(y2, **Cs.CONVERGED)
    d = np.abs(two["T"] - ref["T"]).max()
    assert d <= 1e-9, d
    g0 = Cs.gradient_norm(y, y["T"])
    for precond in (0, 1):
        r = Cs.solve_case(y, mode="pcg", precond=precond)
        dT = np.abs(r["T"] - ref["T"]); gn = Cs.gradient_norm(y, r["T"])
        print("%s precond %d: two starts %.2e apart; dT %.2e chi2 ratio - 1 %.2e gradient %.2e of initial, %d LM / %d PCG iterations"
              % (name, precond, d, dT.max(), r["chi2_final"] / ref["chi2_final"] - 1, gn / g0, r["lm_iters"], r["pcg_iters"]))
        assert np.all(dT <= 0.1 * (1e-6 + 1e-4 * np.abs(ref["T"])))
        assert r["chi2_final"] <= ref["chi2_final"] * (1 + 1e-10)
        assert gn <= 1e-7 * g0
        assert r["chi2_final"] < r["chi2_init"] and r["lm_iters"] < R.DEFAULTS["max_iters"]
        assert np.array_equal(r["T"][hold], g["T"][hold])


def _naive_log(T):
    """a logarithm that knows one sheet of the double cover only: the angle from atan2(|v|, w) in [0, 2 pi), so -q gives a rotation vector of length
    2 pi - theta the other way round"""
    v, w = T[..., :3], T[..., 3]
    n = np.linalg.norm(v, axis=-1)
    om = (2.0 * np.arctan2(n, w) / np.where(n < R.EPS, 1.0, n))[..., None] * v
    return np.concatenate([T[..., 4:], om], -1)


def test_the_input_cases_matter(monkeypatch):
    """For every input case the yardstick with that input IGNORED ends farther from the case's reference than the GPU parity tolerance, so a device
    that ignored it could not pass tests/test_gpu_pose_graph_inputs.py."""
    cases = Cs.input_cases()
    conv = lambda g: Cs.solve_case(g, **Cs.CONVERGED)["T"]
    # fixed dropped.  gauge_mid differs from the default by the gauge alone (every T_k times one transform), so there the held node carries the check:
    # the reference leaves node 6 at its input and moves node 0, the run without `fixed` does the opposite.  gauge_three is another problem.
    g, ref = Cs.input_reference("gauge_mid")
    T = conv(dict(g, fixed=None))
    assert np.array_equal(ref["T"][6], g["T"][6]) and _far(ref["T"][0], g["T"][0]) and _far(T[6], g["T"][6]) and _far(T, ref["T"])
    aligned = R.mul(T, np.broadcast_to(R.mul(R.inverse(T[6]), g["T"][6]), T.shape))
    assert np.allclose(aligned, ref["T"], rtol=0, atol=1e-8)   # (the gauge and nothing else)
    g, ref = Cs.input_reference("gauge_three")
    T = conv(dict(g, fixed=None))
    assert _far(T, ref["T"]) and _far(T[[31, 64]], g["T"][[31, 64]]) and np.array_equal(ref["T"][[0, 31, 64]], g["T"][[0, 31, 64]])
    g, ref = Cs.input_reference("shuffled_hub")
    assert _far(conv(dict(g, fixed=None)), ref["T"])
    assert _far(conv(dict(g, active=(g["ej"] != 0).astype(np.uint8), fixed=Cs.held(65, [0, 64]))), ref["T"])   # (the hub's edges, chain edge (1, 0) with them)
    assert np.bincount(np.concatenate([g["ei"], g["ej"]])).max() >= 41 and (np.diff(g["ei"]) < 0).any()
    # the mask dropped
    g, ref = Cs.input_reference("masked")
    assert _far(conv(dict(g, active=None)), ref["T"])
    # the weight columns taken as [omega; upsilon]
    for name in ("weights", "partial_zero_w"):
        g, ref = Cs.input_reference(name)
        assert _far(conv(Cs.swap_weight_columns(g)), ref["T"]), name
    g, ref = Cs.input_reference("partial_zero_w")
    assert _far(conv(dict(g, w=np.ones_like(g["w"]))), ref["T"])
    # the direction of an edge ignored
    for name in ("reversed", "long_chain_reversed"):
        g, ref = Cs.input_reference(name)
        base = Cs.ring(12, 5) if name == "reversed" else Cs.ring(130, 1)
        rev = g["ei"] != base["ei"]
        assert rev[:len(g["T"]) - 1].any() and not rev[:len(g["T"]) - 1].all() and (name != "reversed" or (rev[11:].any() and not rev[11:].all()))
        assert _far(conv(Cs.swap_ends(g, rev)), ref["T"]), name
    # the sign of a quaternion: the products Z^-1 T_i T_j^-1 reach the other sheet, where a one-sheet logarithm is wrong by 2 pi
    g, ref = Cs.input_reference("quat_signs")
    Em = R.residuals(g["T"], g["ei"], g["ej"], g["Z"])[1]
    assert (Em[:, 3] < 0).any() and (Em[:, 3] > 0).any() and (g["T"][:, 3] < 0).any() and (g["Z"][:, 3] < 0).any()
    plain = Cs.ring_reference(12, 5)[1]["T"]
    sign = np.sign((ref["T"][:, :4] * plain[:, :4]).sum(-1))
    assert (sign < 0).any() and np.allclose(ref["T"] * np.concatenate([sign[:, None].repeat(4, 1), np.ones((12, 3))], -1), plain, rtol=0, atol=1e-9)
    with monkeypatch.context() as m:
        m.setattr(R, "log", _naive_log)
        chi2 = R.edge_chi2(g["T"], g["ei"], g["ej"], g["Z"], g["w"])
    assert np.abs(chi2 - R.edge_chi2(g["T"], g["ei"], g["ej"], g["Z"], g["w"])).max() > 1.0
    # large residuals: with A = I the steps differ, and so does the cost after the first one
    g, ref = Cs.input_reference("large_residuals")
    assert np.abs(R.residuals(g["T"], g["ei"], g["ej"], g["Z"])[0]).max() > 0.3
    first = Cs.solve_case(g, mode="pcg", max_iters=1)
    with monkeypatch.context() as m:
        exact = R.jacobians
        m.setattr(R, "jacobians", lambda r, Em, Zi, exact_A=True: exact(r, Em, Zi, exact_A=False))
        first_I = Cs.solve_case(g, mode="pcg", max_iters=1)
    print("large_residuals: cost after one step %.6e, with A = I %.6e" % (first["chi2_final"], first_I["chi2_final"]))
    assert abs(first_I["chi2_final"] / first["chi2_final"] - 1) > 1e-6
    # a node without information: with ones for its zero weights it would move
    g, ref = Cs.input_reference("zero_weight_node")
    k = Cs.ZERO_WEIGHT_NODE
    assert np.array_equal(ref["T"][k], g["T"][k]) and not Cs.held_of(g)[k] and Cs.held_of(Cs.yardstick_graph("zero_weight_node"))[k]
    assert (g["w"][(g["ei"] == k) | (g["ej"] == k)] == 0).all() and ((g["ei"] == k) | (g["ej"] == k)).sum() >= 2
    assert _far(conv(dict(g, w=np.ones_like(g["w"]))), ref["T"])
    assert set(Cs.INPUT_NAMES) == set(cases)


def test_chain_preconditioner_pays_on_the_reversed_chain():
    """long_chain_reversed: the yardstick's PCG totals under block-Jacobi (c0) and under the chain preconditioner (c1).  The device, told to use the
    chain, must stay under sqrt(c0 c1) (tests/test_gpu_pose_graph_inputs.py): a chain that missed the reversed edges would fall back to c0."""
    c0, c1 = Cs.chain_counts()
    print("long_chain_reversed: %d PCG iterations under block-Jacobi, %d under the chain" % (c0, c1))
    assert c0 >= 3 * c1 and c1 > 0


# ------------------------------------------------------------------------------------------ argument refusals: no GPU needed
def _entry(pkg):
    lib = pkg.load_library()
    return lib, lambda: lib.vslam_last_error().decode()


def test_default_params_and_struct_sizes(pkg):
    p = pkg.default_pose_graph_params()
    assert p.struct_size == C.sizeof(pkg.PoseGraphParams) == 40
    assert (p.max_iters, p.pcg_max_iters, p.pcg_tol, p.step_tol, p.lambda_init) == (50, 4000, 1e-10, 1e-9, 1e-4)
    assert C.sizeof(pkg.PoseGraphBatch) == 16 + 10 * 8 and pkg.POSE_GRAPH_STATS_DTYPE.itemsize == 40
    assert (p.max_iters, p.pcg_max_iters, p.pcg_tol, p.step_tol, p.lambda_init) == tuple(R.DEFAULTS[k] for k in ("max_iters", "pcg_max_iters", "pcg_tol", "step_tol", "lambda_init"))


def test_pose_graph_entries_refuse_bad_arguments(pkg):
    """every refusal comes with VSLAM_ERR_ARG and a message naming its cause, before a context is looked at (so a null context reaches them all)"""
    lib, err = _entry(pkg)
    one = C.c_void_p(8)   # a non-null pointer that is never dereferenced: every call below is refused on the host

    def graph(**kw):
        g = pkg.PoseGraphBatch(struct_size=C.sizeof(pkg.PoseGraphBatch), n_graphs=1, total_nodes=2, total_edges=1, d_node_off=one, d_edge_off=one, d_T=one,
                               d_edge_i=one, d_edge_j=one, d_edge_Z=one, d_edge_w=one)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def call(g, p=None, out=one):
        return lib.vslam_pose_graph_dev(None, C.byref(g) if g is not None else None, C.byref(p) if p is not None else None, out, None)

    assert call(None) == pkg.VSLAM_ERR_ARG and "null graph" in err()
    assert call(graph(struct_size=0)) == pkg.VSLAM_ERR_ARG and "struct_size" in err()
    assert call(graph(struct_size=C.sizeof(pkg.PoseGraphBatch) + 8)) == pkg.VSLAM_ERR_ARG and "struct_size" in err()
    assert call(graph(), pkg.default_pose_graph_params(struct_size=4)) == pkg.VSLAM_ERR_ARG and "vslam_pose_graph_params struct_size" in err()
    for field in ("n_graphs", "total_nodes", "total_edges"):
        assert call(graph(**{field: -1})) == pkg.VSLAM_ERR_ARG and "negative count" in err(), field
    for field in ("d_node_off", "d_edge_off", "d_T", "d_edge_i", "d_edge_j", "d_edge_Z", "d_edge_w"):
        assert call(graph(**{field: None})) == pkg.VSLAM_ERR_ARG and "null d_" in err(), field
    assert call(graph(), out=None) == pkg.VSLAM_ERR_ARG and "d_T_out" in err()
    for kw in (dict(max_iters=-1), dict(pcg_max_iters=0), dict(pcg_tol=-1.0), dict(step_tol=float("nan")), dict(lambda_init=0.0)):
        assert call(graph(), pkg.default_pose_graph_params(**kw)) == pkg.VSLAM_ERR_ARG and "out of range" in err(), kw
    # everything in order but the context
    assert call(graph()) == pkg.VSLAM_ERR_ARG and "null context" in err()
    st = np.zeros(1, np.int32)
    assert lib.vslam_pose_graph_status_dev(None, 1, None) == pkg.VSLAM_ERR_ARG and "null h_status" in err()
    assert lib.vslam_pose_graph_status_dev(None, -1, st) == pkg.VSLAM_ERR_ARG and "negative" in err()
    assert lib.vslam_pose_graph_status_dev(None, 1, st) == pkg.VSLAM_ERR_ARG and "null context" in err()


def test_pg_precond_is_a_tuning_key():
    """the key is on the library's table: its name and its environment variable are in the binary"""
    import stereo_visual_slam_amd as pkg
    blob = open(pkg._SO, "rb").read()
    assert b"pg_precond" in blob and b"VSLAM_PG_PRECOND" in blob
