"""Seeded pose graphs for the pose-graph tests: rings with drift and loop edges, and the degenerate graphs the entry must take as results.
A graph is dict(T (N, 7), ei, ej (E), Z (E, 7), w (E, 6), fixed (N uint8 or None), active (E uint8 or None)); pack() lays several back to back.
The rings vary the size; input_cases() varies what a graph may say besides: held nodes, the mask, weights, edge direction and order, quaternion signs."""
import functools

import numpy as np

import pose_graph_ref as R

RING_NODES = (2, 12, 65, 130)
RING_LOOPS = (1, 5, 30)
# the yardstick's converged poses are taken past the library's default stop (step_tol 1e-9), and polished to the rounding floor of the gradient, so that what
# is left of its own iteration does not count against the device
CONVERGED = dict(step_tol=1e-13, max_iters=100, polish=5)


def _noise(rng, n, s_t, s_r):
    return R.exp(np.concatenate([rng.normal(0, s_t, (n, 3)), rng.normal(0, s_r, (n, 3))], -1))


def ring(N, L, seed=0, s_t=0.004, s_r=0.002, w_odo=(1.0, 1.0), w_loop=(1.0, 1.0)):
    """A camera that drives one lap (0.1 m per node, looking along the tangent) and comes back to its start.  Odometry edges (k + 1, k) carry noise;
    the initial poses chain them from node 0 and so drift; L loop edges (q, c), q > c, tie late nodes to early ones with noise of the same size.
    The lap is kept small on purpose: a 130-node ring with one loop edge is so weakly tied that, at 0.5 m per node (poses 10 m from the origin), the
    rounding of the cost alone moves the yardstick's end point by 3e-8, more than the 1e-9 its two-start guard allows."""
    rng = np.random.default_rng(1000 * N + 10 * L + seed)
    ang = 2 * np.pi * np.arange(N) / max(N, 2)
    rad = 0.1 * max(N, 2) / (2 * np.pi)
    # T_w_c: position on the circle, yaw about y; then T_c_w
    Twc = np.zeros((N, 7))
    Twc[:, 1] = np.sin(-ang / 2); Twc[:, 3] = np.cos(-ang / 2)
    Twc[:, 4] = rad * np.sin(ang); Twc[:, 5] = 0.01 * np.sin(3 * ang); Twc[:, 6] = rad * (1 - np.cos(ang))
    Tt = R.inverse(Twc)
    ei = np.arange(1, N); ej = np.arange(0, N - 1)
    Zo = R.mul(_noise(rng, N - 1, s_t, s_r), R.mul(Tt[ei], R.inverse(Tt[ej])))
    T0 = np.zeros((N, 7)); T0[0] = Tt[0]
    for k in range(1, N):
        T0[k] = R.mul(Zo[k - 1], T0[k - 1])
    gap = min(2, N - 1)
    lq = rng.integers(gap, N, L); lc = np.floor(rng.random(L) * (lq - gap + 1)).astype(np.int64)   # (c <= q - gap; an edge may come twice)
    Zl = R.mul(_noise(rng, L, s_t, s_r), R.mul(Tt[lq], R.inverse(Tt[lc])))
    w = np.concatenate([np.tile(np.repeat(w_odo, 3), (N - 1, 1)), np.tile(np.repeat(w_loop, 3), (L, 1))])
    return dict(T=T0, ei=np.concatenate([ei, lq]).astype(np.int32), ej=np.concatenate([ej, lc]).astype(np.int32), Z=np.concatenate([Zo, Zl]), w=w,
                fixed=None, active=None, T_true=Tt)


def perturbed(g, seed, sigma=0.02):
    """the second start of the yardstick guard: every free pose moved by exp(N(0, sigma))"""
    rng = np.random.default_rng(seed)
    T = g["T"].copy()
    free = ~R.held_nodes(len(T), g["ei"], g["ej"], g["fixed"], R._active(len(g["ei"]), g["active"]))
    T[free] = R.mul(R.exp(rng.normal(0, sigma, (int(free.sum()), 6))), T[free])
    return dict(g, T=T)


def degenerate():
    """{name: (graph, expected n_free)}: every one is a result, status 0, finite output"""
    base = ring(12, 5, seed=3)
    e = dict(ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), Z=np.zeros((0, 7)), w=np.zeros((0, 6)), fixed=None, active=None)
    out = {}
    out["no_nodes"] = (dict(e, T=np.zeros((0, 7))), 0)
    out["one_node"] = (dict(e, T=base["T"][:1].copy()), 0)
    out["no_edges"] = (dict(e, T=base["T"][:5].copy()), 0)
    out["all_fixed"] = (dict(base, fixed=np.ones(12, np.uint8)), 0)
    # no edge between nodes 5 and 6, but loop edges across the break
    keep = ~((base["ei"] == 6) & (base["ej"] == 5))
    out["broken_chain"] = (dict(base, ei=base["ei"][keep], ej=base["ej"][keep], Z=base["Z"][keep], w=base["w"][keep]), 11)
    # nodes 8..11 are tied to each other only: no path to the fixed node 0, the component moves under damping alone
    keep = ~(((base["ei"] >= 8) & (base["ej"] < 8)) | ((base["ei"] < 8) & (base["ej"] >= 8)))
    out["floating_component"] = (dict(base, ei=base["ei"][keep], ej=base["ej"][keep], Z=base["Z"][keep], w=base["w"][keep]), 11)
    # every loop edge switched off through the mask: the chain alone, which the initial poses already satisfy
    act = np.ones(len(base["ei"]), np.uint8); act[11:] = 0
    out["loops_inactive"] = (dict(base, active=act), 11)
    return out


def pack(graphs):
    """(T, node_off, edges dict, fixed or None, active or None) of graphs laid back to back"""
    node_off = np.cumsum([0] + [len(g["T"]) for g in graphs]).astype(np.int32)
    edge_off = np.cumsum([0] + [len(g["ei"]) for g in graphs]).astype(np.int32)
    cat = lambda k, shape, dt: np.concatenate([np.asarray(g[k], dt).reshape(shape) for g in graphs]) if graphs else np.zeros(shape, dt).reshape(shape)
    edges = dict(off=edge_off, i=cat("ei", (-1,), np.int32), j=cat("ej", (-1,), np.int32), Z=cat("Z", (-1, 7), np.float64), w=cat("w", (-1, 6), np.float64))
    fixed = active = None
    if any(g["fixed"] is not None for g in graphs):
        fixed = np.concatenate([np.asarray(g["fixed"], np.uint8) if g["fixed"] is not None else (np.arange(len(g["T"])) == 0).astype(np.uint8) for g in graphs])
    if any(g["active"] is not None for g in graphs):
        active = np.concatenate([np.asarray(g["active"], np.uint8) if g["active"] is not None else np.ones(len(g["ei"]), np.uint8) for g in graphs])
    return cat("T", (-1, 7), np.float64), node_off, edges, fixed, active


@functools.lru_cache(maxsize=None)
def ring_reference(N, L):
    """(graph, the yardstick's converged result): computed once, shared by the CPU guard and the GPU tests, never modified"""
    g = ring(N, L)
    ref = R.solve(g["T"], g["ei"], g["ej"], g["Z"], g["w"], **CONVERGED)
    for v in list(g.values()) + [ref["T"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g, ref


def gradient_norm(g, T):
    return float(np.linalg.norm(R.cost_and_gradient(T, g["ei"], g["ej"], g["Z"], g["w"], g["fixed"], g["active"])[1]))


# ------------------------------------------------------------------------------------------ the input space: masks, held nodes, weights, directions
def held(N, nodes):
    f = np.zeros(N, np.uint8); f[list(nodes)] = 1
    return f


def reverse_edges(g, which):
    """a copy whose edges `which` (a mask over the edges) are stored the other way round, (j, i, Z^-1): the same measurement"""
    which = np.asarray(which, bool)
    ei, ej, Z = g["ei"].copy(), g["ej"].copy(), g["Z"].copy()
    ei[which], ej[which] = g["ej"][which], g["ei"][which]
    Z[which] = R.inverse(g["Z"][which])
    return dict(g, ei=ei, ej=ej, Z=Z)


def swap_ends(g, which):
    """what a reader that ignores the direction makes of it: the edges `which` with i and j exchanged and Z as it stands"""
    which = np.asarray(which, bool)
    ei, ej = g["ei"].copy(), g["ej"].copy()
    ei[which], ej[which] = g["ej"][which], g["ei"][which]
    return dict(g, ei=ei, ej=ej)


def swap_weight_columns(g):
    """what a reader that takes the information as [omega; upsilon] makes of it"""
    return dict(g, w=np.concatenate([g["w"][:, 3:], g["w"][:, :3]], -1))


def without_edges_at(g, node):
    """a copy with every edge at `node` switched off through the mask (the node is then held)"""
    act = R._active(len(g["ei"]), g["active"]) & (g["ei"] != node) & (g["ej"] != node)
    return dict(g, active=act.astype(np.uint8))


def flip_quaternions(g, seed):
    """-q on about half of the poses and half of the measurements: the same rotations on the other sheet of the double cover"""
    rng = np.random.default_rng(seed)
    T, Z = g["T"].copy(), g["Z"].copy()
    nt, nz = rng.random(len(T)) < 0.5, rng.random(len(Z)) < 0.5
    nt[1], nz[0] = True, True
    T[nt, :4] *= -1.0; Z[nz, :4] *= -1.0
    return dict(g, T=T, Z=Z)


ZERO_WEIGHT_NODE = 6


@functools.lru_cache(maxsize=None)
def input_cases():
    """{name: graph} of the cases that vary what the rings leave alone: which nodes are held, the edge mask, weights per edge and component, the
    direction and order of the edges, the sign of the quaternions, the size of the residuals.  Every one is well posed but zero_weight_node, whose
    node ZERO_WEIGHT_NODE is free yet has no information (the library's VSLAM_PG_SINGULAR); input_reference() says what it is compared with."""
    base = ring(12, 5)
    E = len(base["ei"])
    rng = np.random.default_rng(4242)
    out = {}
    out["gauge_mid"] = dict(base, fixed=held(12, [6]))                     # node 0 is free
    out["gauge_three"] = dict(ring(65, 5), fixed=held(65, [0, 31, 64]))    # held nodes in mid-chain and at its end
    out["weights"] = dict(base, w=np.exp(rng.uniform(np.log(0.25), np.log(400.0), (E, 6))))
    rev = rng.random(E) < 0.5
    rev[[0, 3, 11]] = True; rev[[1, 12]] = False                           # (chain and loop edges on both sides, whatever the draw)
    out["reversed"] = reverse_edges(base, rev)
    # 65-node ring with one loop edge, 40 more edges at node 0, node 64 held, the edges in random order
    hub = ring(65, 1)
    hq = np.sort(rng.choice(np.arange(2, 65), 40, replace=False))
    Zh = R.mul(_noise(rng, 40, 0.004, 0.002), R.mul(hub["T_true"][hq], R.inverse(hub["T_true"][np.zeros(40, np.int64)])))
    hub = dict(hub, ei=np.concatenate([hub["ei"], hq]).astype(np.int32), ej=np.concatenate([hub["ej"], np.zeros(40)]).astype(np.int32),
               Z=np.concatenate([hub["Z"], Zh]), w=np.concatenate([hub["w"], np.ones((40, 6))]), fixed=held(65, [64]))
    order = rng.permutation(len(hub["ei"]))
    out["shuffled_hub"] = dict(hub, ei=hub["ei"][order], ej=hub["ej"][order], Z=hub["Z"][order], w=hub["w"][order])
    out["quat_signs"] = flip_quaternions(base, 17)
    w = base["w"].copy(); w[11:, 3:] = 0.0                                  # the loop edges measure no rotation; the chain keeps the graph well posed
    out["partial_zero_w"] = dict(base, w=w)
    act = np.ones(E, np.uint8); act[[4, 11, 15]] = 0                        # chain edge (5, 4) and two loop edges; loop edge (7, 0) spans the break
    out["masked"] = dict(base, active=act)
    out["large_residuals"] = ring(12, 5, s_t=0.1, s_r=0.15)
    # one loop edge on 130 nodes, every second chain edge stored the other way round: the chain preconditioner must still see them all
    lc = ring(130, 1)
    every_second = np.zeros(len(lc["ei"]), bool); every_second[0:129:2] = True
    out["long_chain_reversed"] = reverse_edges(lc, every_second)
    w = base["w"].copy(); w[(base["ei"] == ZERO_WEIGHT_NODE) | (base["ej"] == ZERO_WEIGHT_NODE)] = 0.0
    out["zero_weight_node"] = dict(base, w=w)
    for g in out.values():
        for v in g.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


WELL_POSED_INPUT_NAMES = ["gauge_mid", "gauge_three", "weights", "reversed", "shuffled_hub", "quat_signs", "partial_zero_w", "masked", "large_residuals",
                          "long_chain_reversed"]
INPUT_NAMES = WELL_POSED_INPUT_NAMES + ["zero_weight_node"]


def yardstick_graph(name):
    """the graph the yardstick solves for a case: the case itself, but for zero_weight_node the graph without that node's edges (a singular H has no
    dense solve; the library leaves the node where it is, which is what holding it does)"""
    g = input_cases()[name]
    return without_edges_at(g, ZERO_WEIGHT_NODE) if name == "zero_weight_node" else g


@functools.lru_cache(maxsize=None)
def input_reference(name):
    """(graph, the yardstick's converged result on yardstick_graph(name)): computed once, shared by the CPU guard and the GPU tests, never modified"""
    g, y = input_cases()[name], yardstick_graph(name)
    ref = R.solve(y["T"], y["ei"], y["ej"], y["Z"], y["w"], y["fixed"], y["active"], **CONVERGED)
    ref["T"].setflags(write=False)
    return g, ref


@functools.lru_cache(maxsize=None)
def chain_counts():
    """(c0, c1): the yardstick's PCG iteration totals on long_chain_reversed at the library's defaults, under block-Jacobi and under the chain"""
    g = input_cases()["long_chain_reversed"]
    return tuple(solve_case(g, mode="pcg", precond=p)["pcg_iters"] for p in (0, 1))


def solve_case(g, **kw):
    return R.solve(g["T"], g["ei"], g["ej"], g["Z"], g["w"], g["fixed"], g["active"], **kw)


def held_of(g):
    return R.held_nodes(len(g["T"]), g["ei"], g["ej"], g["fixed"], R._active(len(g["ei"]), g["active"]))
