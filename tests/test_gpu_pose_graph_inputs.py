"""GPU: pose_graph_kernel (vslam_pose_graph_dev) over its input space -- held nodes anywhere, the edge mask, weights per edge and component, edges
stored either way round and in any order, quaternions on either sheet, large residuals, a node without information, the rule that picks the
preconditioner, in-place output -- against the numpy yardstick of tests/pose_graph_ref.py.  tests/test_gpu_pose_graph.py covers the sizes; the
cases are tests/pose_graph_cases.py input_cases(), and tests/test_pose_graph_ref.py guards every one of them and every bound asserted here."""
import numpy as np
import pytest

import pose_graph_cases as Cs
import pose_graph_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("T", "edge_chi2", "stats")


def run(vo, graphs, precond=-1, **params):
    T, node_off, edges, fixed, active = Cs.pack(graphs)
    vo.set_tuning(pg_precond=precond)
    try:
        return vo.optimize_pose_graph(T, node_off, edges, fixed=fixed, active=active, **params)
    finally:
        vo.set_tuning(pg_precond=-1)


def split(out, graphs):
    """the per-graph slices (T, edge_chi2, stats record) of a batch result"""
    n = np.cumsum([0] + [len(g["T"]) for g in graphs]); e = np.cumsum([0] + [len(g["ei"]) for g in graphs])
    return [(out["T"][n[k]:n[k + 1]], out["edge_chi2"][e[k]:e[k + 1]], out["stats"][k]) for k in range(len(graphs))]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def check_parity(g, ref, T, chi2, st, label, max_iters=R.DEFAULTS["max_iters"]):
    """the bounds of tests/test_gpu_pose_graph.py on one graph: chi2 values against numpy at the device's poses at rtol 1e-9 (of every edge, the masked
    ones too), poses within rtol 1e-4 / atol 1e-6 of the yardstick's converged ones, the exact gradient at most 1e-6 of the initial one, the cost
    fallen; and held nodes exactly where they were.
    The absolute term of the per-edge comparison: a residual component is the end of two products, an inverse and a logarithm of poses of order one, so
    it carries some d = 1e-15 of absolute rounding (eps 2.2e-16) on either side, and chi2 = r' W r then 2 sqrt(w chi2) d + 6 w d^2.  That exceeds
    1e-9 chi2 only where chi2 < 4e-12 w: at edges whose residual the optimiser has driven to zero (the chain past the last loop edge), where a relative
    bound alone would compare rounding with rounding."""
    want = R.edge_chi2(T, g["ei"], g["ej"], g["Z"], g["w"])
    chi2_atol = 2e-15 * np.sqrt(g["w"].max(-1) * want) + 6e-30 * g["w"].max(-1)
    cost, grad = R.cost_and_gradient(T, g["ei"], g["ej"], g["Z"], g["w"], g["fixed"], g["active"])
    g0 = Cs.gradient_norm(g, g["T"])
    print("%s: chi2 %.9e -> %.9e (numpy at the device's poses %.9e, yardstick %.9e), gradient %.2e of initial, max |dT| %.2e, %d LM / %d PCG iterations, status %d"
          % (label, st["chi2_init"], st["chi2_final"], cost, ref["chi2_final"], np.linalg.norm(grad) / g0, np.abs(T - ref["T"]).max(), st["lm_iters"],
             st["pcg_iters"], st["status"]))
    assert np.isclose(st["chi2_init"], ref["chi2_init"], rtol=1e-9, atol=0)
    assert np.isclose(st["chi2_final"], cost, rtol=1e-9, atol=0)
    assert np.all(np.abs(chi2 - want) <= 1e-9 * want + chi2_atol)
    assert np.allclose(T, ref["T"], rtol=1e-4, atol=1e-6)
    assert st["chi2_final"] <= ref["chi2_final"] * (1 + 1e-9)
    assert np.linalg.norm(grad) <= 1e-6 * g0
    assert st["chi2_final"] < st["chi2_init"]
    assert 0 < st["lm_iters"] < max_iters
    hold = Cs.held_of(g)
    assert np.array_equal(T[hold], g["T"][hold])


def test_evaluation_only(vo):
    """max_iters = 0 on one batch of four graphs of which one has a mask: chi2_init and the chi2 of EVERY edge against numpy at rtol 1e-9, the masked
    edges left out of chi2_init, the poses copied.  The free poses are moved first, so that no residual is zero and a relative bound means something."""
    cases = Cs.input_cases()
    graphs = [Cs.perturbed(cases[name], 11 + k) for k, name in enumerate(("weights", "reversed", "quat_signs", "masked"))]
    out = run(vo, graphs, max_iters=0)
    for g, (T, chi2, st) in zip(graphs, split(out, graphs)):
        want = R.edge_chi2(g["T"], g["ei"], g["ej"], g["Z"], g["w"])
        act = R._active(len(want), g["active"])
        assert want.min() > 1e-6
        assert np.array_equal(T, g["T"])
        assert np.allclose(chi2, want, rtol=1e-9, atol=0)
        assert np.isclose(st["chi2_init"], want[act].sum(), rtol=1e-9, atol=0) and st["chi2_final"] == st["chi2_init"]
        assert (st["lm_iters"], st["pcg_iters"], st["status"], st["n_free"]) == (0, 0, 0, 11)
    g = graphs[3]
    assert (~R._active(len(g["ei"]), g["active"])).sum() == 3 and not np.isclose(split(out, graphs)[3][2]["chi2_init"], split(out, graphs)[3][1].sum(), rtol=1e-3)


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", Cs.WELL_POSED_INPUT_NAMES)
def test_parity(vo, name, precond):
    g, ref = Cs.input_reference(name)
    T, chi2, st = split(run(vo, [g], precond), [g])[0]
    check_parity(g, ref, T, chi2, st, "%s precond %d" % (name, precond))
    assert st["status"] == 0 and st["n_free"] == ref["n_free"]
    if name == "quat_signs":   # the same answer as without the flips, up to the sign of each quaternion
        plain = Cs.ring_reference(12, 5)[1]["T"]
        sign = np.where((T[:, :4] * plain[:, :4]).sum(-1) < 0, -1.0, 1.0)
        assert (sign < 0).any() and (sign > 0).any()
        assert np.allclose(np.concatenate([T[:, :4] * sign[:, None], T[:, 4:]], -1), plain, rtol=1e-4, atol=1e-6)
    if name == "long_chain_reversed" and precond == 1:
        c0, c1 = Cs.chain_counts()
        print("   PCG iterations: yardstick %d under block-Jacobi, %d under the chain; the device under the chain %d" % (c0, c1, st["pcg_iters"]))
        assert st["pcg_iters"] < np.sqrt(c0 * c1)


@pytest.mark.parametrize("precond", [0, 1])
def test_a_node_without_information_stays_where_it_is(vo, pkg, precond):
    """zero_weight_node: node 6 is free but all its edges weigh nothing, so its block of H is zero.  Status exactly VSLAM_PG_SINGULAR, finite output, the
    node within 1e-12 of its input (se3::mul renormalises, so not bytes), and the rest of the graph as the yardstick finds it without that node's edges."""
    g, ref = Cs.input_reference("zero_weight_node")
    k = Cs.ZERO_WEIGHT_NODE
    T, chi2, st = split(run(vo, [g], precond), [g])[0]
    assert st["status"] == pkg.PG_SINGULAR and st["n_free"] == 11 == ref["n_free"] + 1
    assert np.isfinite(T).all() and np.isfinite(chi2).all() and np.isfinite(st["chi2_final"])
    assert np.abs(T[k] - g["T"][k]).max() <= 1e-12
    check_parity(g, ref, T, chi2, st, "zero_weight_node precond %d" % precond)


def test_the_rule_counts_active_edges_off_the_chain(vo):
    """pg_precond = -1 on a 65-node ring: the chain preconditioner up to 16 active edges off the chain, block-Jacobi from 17; an edge the mask
    switches off does not count.  Told by the bytes, which differ between the two preconditioners."""
    g16, g17 = Cs.ring(65, 16), Cs.ring(65, 17)
    act = np.ones(len(g17["ei"]), np.uint8); act[-1] = 0
    g17m = dict(g17, active=act)
    for g, want in ((g16, 1), (g17, 0), (g17m, 1)):
        d = g["ei"].astype(np.int64) - g["ej"]
        assert ((np.abs(d) != 1) & R._active(len(d), g["active"])).sum() == (17 if want == 0 else 16)
        by_rule, forced = run(vo, [g], -1), {p: run(vo, [g], p) for p in (0, 1)}
        assert (forced[0]["stats"]["status"] == 0).all() and (forced[1]["stats"]["status"] == 0).all()
        assert not same_bytes(forced[0], forced[1]) and forced[0]["stats"]["pcg_iters"][0] != forced[1]["stats"]["pcg_iters"][0]
        assert same_bytes(by_rule, forced[want]), want


def _batches():
    """three graphs of different sizes: `fixed` and an edge mask on the middle one only, and on all but the first"""
    cases = Cs.input_cases()
    plain12, plain130 = Cs.ring(12, 5, seed=2), Cs.ring(130, 5)
    mid = cases["gauge_three"]
    act = np.ones(len(mid["ei"]), np.uint8); act[[64, 66]] = 0   # two of its five loop edges
    mid = dict(mid, active=act)
    last = dict(cases["masked"], fixed=Cs.held(12, [6]))
    return [plain12, mid, plain130], [plain12, mid, last]


@pytest.mark.parametrize("precond", [0, 1])
def test_masks_and_held_nodes_in_a_batch(vo, precond):
    """the same call twice gives the same bytes, and every graph is bit for bit its output alone, where its own call passes NULL for what the batch
    had to fill in for it (node 0 held, every edge active)"""
    for graphs in _batches():
        assert sum(g["fixed"] is None for g in graphs) in (1, 2) and len({len(g["T"]) for g in graphs}) >= 2
        out = run(vo, graphs, precond)
        assert same_bytes(out, run(vo, graphs, precond))
        assert (out["stats"]["status"] == 0).all() and (out["stats"]["lm_iters"] > 0).all()
        for k, (g, part) in enumerate(zip(graphs, split(out, graphs))):
            alone = split(run(vo, [g], precond), [g])[0]
            for a, b in zip(part, alone):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (precond, k)
            assert np.array_equal(part[0][Cs.held_of(g)], g["T"][Cs.held_of(g)]) and part[2]["n_free"] == int((~Cs.held_of(g)).sum())


@pytest.mark.parametrize("precond", [0, 1])
def test_in_place(vo, pkg, precond):
    """vslam_pose_graph_dev with d_T_out = d_T: the bytes of the call with an output of its own, on three graphs of which one is masked"""
    import torch
    graphs = _batches()[0]
    T, node_off, edges, fixed, active = Cs.pack(graphs)
    want = run(vo, graphs, precond)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for in_place in (False, True):
        t = dict(node_off=up(node_off), edge_off=up(edges["off"]), T=up(T), ei=up(edges["i"]), ej=up(edges["j"]), Z=up(edges["Z"]), w=up(edges["w"]),
                 fixed=up(fixed), active=up(active), chi2=torch.zeros(len(edges["i"]), dtype=torch.float64, device=dev),
                 stats=torch.zeros(3 * pkg.POSE_GRAPH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        t["out"] = t["T"] if in_place else torch.zeros_like(t["T"])
        b = pkg.PoseGraphBatch(n_graphs=3, total_nodes=len(T), total_edges=len(edges["i"]), d_node_off=t["node_off"].data_ptr(), d_edge_off=t["edge_off"].data_ptr(),
                               d_T=t["T"].data_ptr(), d_fixed=t["fixed"].data_ptr(), d_edge_i=t["ei"].data_ptr(), d_edge_j=t["ej"].data_ptr(),
                               d_edge_Z=t["Z"].data_ptr(), d_edge_w=t["w"].data_ptr(), d_edge_active=t["active"].data_ptr(), d_edge_chi2=t["chi2"].data_ptr())
        torch.cuda.synchronize()
        vo.set_tuning(pg_precond=precond)
        try:
            vo.pose_graph_dev(b, None, t["out"].data_ptr(), t["stats"].data_ptr())
            vo.sync()
        finally:
            vo.set_tuning(pg_precond=-1)
        got = dict(T=t["out"].cpu().numpy(), edge_chi2=t["chi2"].cpu().numpy(), stats=t["stats"].cpu().numpy().view(pkg.POSE_GRAPH_STATS_DTYPE))
        assert (t["out"].data_ptr() == t["T"].data_ptr()) == in_place
        assert same_bytes(got, want), in_place
    assert (want["stats"]["status"] == 0).all() and not np.array_equal(want["T"], T)
