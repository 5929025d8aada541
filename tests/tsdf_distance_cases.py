"""Inputs of the clearance layer's tests (tests/test_tsdf_distance_ref.py on the CPU, tests/test_gpu_tsdf_distance.py on the device): hand-made
fields that go in through TsdfMap.load_blocks, and two integrated scenes of tests/tsdf_cases.py.  A case is a dump (ids, vox), the voxel size and the
builds to run on it: (map_id, min_weight, radius, log2_layer_blocks).  The hand-worked numbers of (a), (d) and (f) are written here."""
import functools

import numpy as np

import tsdf_distance_ref as DR

FREE_V = (1, 1536, 1, 0)       # num = 1536 - 1024 > 0
OCC_V = (1, 512, 1, 0)         # num = 512 - 1024 <= 0
VS = 0.2
LOG2_POOL = 10                 # the TsdfMap the hand-made fields are loaded into
EDGE = 1 << 17


def field(voxels):
    """{(map, ix, iy, iz): (W, Sq, Wc, I)} -> a dump (ids (n, 4) int32, vox (n, 512, 4) uint32) sorted by (map, bx, by, bz)"""
    blocks = {}
    for (m, ix, iy, iz), v in voxels.items():
        blk = blocks.setdefault((m, ix >> 3, iy >> 3, iz >> 3), np.zeros((512, 4), np.uint32))
        blk[(iz & 7) << 6 | (iy & 7) << 3 | (ix & 7)] = v
    keys = sorted(blocks)
    return np.array(keys, np.int32).reshape(-1, 4), (np.stack([blocks[k] for k in keys]) if keys else np.zeros((0, 512, 4), np.uint32))


def _build(map_id=-1, min_weight=1, radius=8, log2=10):
    return dict(map_id=map_id, min_weight=min_weight, radius=radius, log2=log2)


def _case(name, voxels, builds, points=(), voxel_size=VS):
    ids, vox = field(voxels)
    return dict(name=name, ids=ids, vox=vox, voxel_size=voxel_size, builds=list(builds), points=np.asarray(points, np.float64).reshape(-1, 3), scene=None)


def _with_free(sites, m=0, d=(0, 1, 0)):
    """every site OCCUPIED with a FREE voxel at + d"""
    v = {}
    for s in sites:
        v[(m,) + tuple(int(c) for c in s)] = OCC_V
    for s in sites:
        v.setdefault((m,) + tuple(int(c) + e for c, e in zip(s, d)), FREE_V)
    return v


def _axis_sites(shift=(0, 0, 0)):
    """(b): a site at voxel index 7, 8, -1 and -8 on each axis (the other two coordinates 3), the block boundaries on both sides of zero"""
    out = []
    for a in range(3):
        for p in (7, 8, -1, -8):
            s = [3 + shift[0], 3 + shift[1], 3 + shift[2]]
            s[a] = p + shift[a]
            out.append(tuple(s))
    return out


# (d) the separable-pass trap: four sites around a probe, none of them nearest on every axis.  With all four the probe's d2 is 25; without the first
# 27; without the first two 32; with the last alone 36.
PROBE = (20, 20, 20)
TRAP = [(5, 0, 0), (3, 3, 3), (4, 4, 0), (0, 0, 6)]
TRAP_D2 = [25, 27, 32, 36]
# (a) the single site at the origin: |v|^2 of some voxels, which is their d2 where it does not exceed R^2.  At R = 7 the ball spans the eight blocks
# that meet at the origin; at R = 8 voxel index 8 on each axis adds three more.
ONE_SITE_NORM2 = {(0, 0, 0): 0, (-1, 0, 0): 1, (3, -4, 0): 25, (-7, 0, 0): 49, (-8, 0, 0): 64, (8, 0, 0): 64, (-5, -5, -4): 66, (8, 1, 0): 65, (7, 3, 2): 62, (4, 4, 4): 48}
# (f) sites by min_weight: an OCCUPIED voxel without a FREE neighbour is none; one whose FREE neighbour has W = 1 is one at min_weight 1 only; the W = 2
# pair is one at both; a voxel at W = 2^20 is not good, so neither a site nor classed
NOT_A_SITE = {(0, 2, 2, 2): OCC_V,
              (0, 10, 2, 2): (2, 1024, 2, 0), (0, 11, 2, 2): FREE_V,
              (0, 20, 2, 2): (2, 1024, 2, 0), (0, 21, 2, 2): (2, 3072, 2, 0),
              (0, 30, 2, 2): (1 << 20, 1 << 29, 1, 0), (0, 31, 2, 2): FREE_V}
NOT_A_SITE_EXPECT = {1: [(10, 2, 2), (20, 2, 2)], 2: [(20, 2, 2)]}


def _random_sparse(seed=3, n=200, side=24):
    rng = np.random.default_rng(seed)
    flat = rng.choice(side ** 3, n, replace=False)
    occ = np.stack([flat % side, (flat // side) % side, flat // (side * side)], 1)
    v = {(0,) + tuple(int(c) for c in s): OCC_V for s in occ}
    for s in occ:
        a, d = int(rng.integers(3)), int(rng.choice((-1, 1)))
        t = [int(c) for c in s]
        t[a] += d
        v.setdefault((0,) + tuple(t), FREE_V)      # (an OCCUPIED voxel there stays: that neighbour is then no free one)
    return v


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    one = {(0, 0, 0, 0): OCC_V, (0, -1, 0, 0): FREE_V}
    out.append(_case("a_one_site", one, [_build(radius=7), _build(radius=8)], points=[(0.1, 0.1, 0.1), (-0.1, 0.1, 0.1), (-1.7, 0.0, 0.0), (1.65, 0.3, 0.1)]))
    axis = _with_free(_axis_sites())
    out.append(_case("b_block_edges", axis, [_build()]))
    out.append(_case("c_radii", axis, [_build(radius=r) for r in (1, 7, 9, 16)]))     # (R = 8 is case b)
    for k in range(4):
        sites = [tuple(p + o for p, o in zip(PROBE, off)) for off in TRAP[k:]]
        out.append(_case("d_trap_%d" % TRAP_D2[k], _with_free(sites), [_build(radius=6), _build(radius=16)]))
    out.append(_case("d_random_sparse", _random_sparse(), [_build(radius=5), _build(radius=8)]))
    two = dict(_with_free(_axis_sites(), m=0))
    two.update(_with_free(_axis_sites((1, 0, 0)), m=5))
    out.append(_case("e_two_maps", two, [_build(), _build(map_id=0), _build(map_id=5)]))
    out.append(_case("f_not_a_site", NOT_A_SITE, [_build(min_weight=1, radius=4), _build(min_weight=2, radius=4), _build(min_weight=0, radius=4)]))
    hi, lo = EDGE - 1, -EDGE
    edge = {(0, hi, 0, 0): OCC_V, (0, hi - 1, 0, 0): FREE_V, (0, 5, lo, 5): OCC_V, (0, 5, lo + 1, 5): FREE_V, (0, hi, hi, lo): OCC_V, (0, hi, hi, lo + 1): FREE_V}
    vs = float(np.float32(VS))
    out.append(_case("g_range_edges", edge, [_build(radius=8), _build(radius=16)],
                     points=[((hi + 0.5) * vs, 0.1, 0.1), (EDGE * vs, 0.1, 0.1), ((hi + 1.5) * vs, 0.1, 0.1), (1.1, (lo + 0.5) * vs, 1.1), (1.1, (lo - 0.5) * vs, 1.1),
                             ((hi - 3 + 0.5) * vs, (hi - 2 + 0.5) * vs, (lo + 4.5) * vs)]))
    out.append(_case("h_empty", {}, [_build()]))
    no_site = {(2, 1, 1, 1): FREE_V, (2, 2, 1, 1): FREE_V, (2, 40, 1, 1): (0, 0, 0, 0), (2, 41, 1, 1): OCC_V}
    out.append(_case("h_no_site", no_site, [_build(), _build(radius=16)]))
    out.append(_case("i_overflow", one, [_build(radius=16, log2=6), _build(radius=8, log2=6)]))    # 125 blocks into 64 slots: void; then 27: served
    for name, radii in (("scene", (3, 8)), ("narrow", (3, 8))):
        c = dict(name="k_" + name, ids=None, vox=None, voxel_size=None, builds=[_build(radius=r, log2=12) for r in radii], points=np.zeros((0, 3)), scene=name)
        out.append(c)
    return {c["name"]: c for c in out}


@functools.lru_cache(maxsize=None)
def dump_of(name):
    """the case's dump and voxel size: hand-made, or the restatement of the integrated scene of tests/tsdf_cases.py (shared, do not change it)"""
    c = cases()[name]
    if c["scene"] is None:
        return c["ids"], c["vox"], c["voxel_size"]
    import tsdf_cases as TC
    ids, vox = TC.reference_of(c["scene"]).dump()
    return ids, vox, TC.cases()[c["scene"]]["voxel_size"]


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """the yardstick's layer of build k of a case, computed once and shared: do not change it"""
    ids, vox, _ = dump_of(name)
    b = cases()[name]["builds"][k]
    return DR.layer(ids, vox, b["map_id"], b["min_weight"], b["radius"], b["log2"])


def query_points(name, k, n=4096, seed=0):
    """the points of a case's query test: random ones in the layer's bounding box grown by R + 2 voxels (the origin's surroundings for an empty layer),
    points exactly on voxel faces, non-finite ones, ones out of range, the case's own; with map ids, some of them wrong"""
    _, _, voxel_size = dump_of(name)
    lay, b = reference(name, k), cases()[name]["builds"][k]
    vs = float(np.float32(voxel_size))
    rng = np.random.default_rng(seed + k)
    ids = lay["ids"] if len(lay["ids"]) else np.array([[0, 0, 0, 0]], np.int32)
    grow = b["radius"] + 2
    lo = (ids[:, 1:].min(0).astype(np.float64) * 8 - grow) * vs
    hi = (ids[:, 1:].max(0).astype(np.float64) * 8 + 8 + grow) * vs
    extra = cases()[name]["points"]
    n_rand = n - 1024 - 64 - 64 - len(extra)
    pts = [rng.uniform(lo, hi, (n_rand, 3))]
    # near the sites, where most of the layer's information is
    faces = np.rint(rng.uniform(lo, hi, (1024, 3)) / vs) * vs            # k * vs: exactly on a voxel face
    faces[512:, 1:] += rng.uniform(0, vs, (512, 2))
    pts.append(faces)
    bad = rng.uniform(lo, hi, (64, 3))
    bad[np.arange(64), rng.integers(0, 3, 64)] = rng.choice([np.nan, np.inf, -np.inf], 64)
    pts.append(bad)
    far = rng.uniform(lo, hi, (64, 3))
    far[np.arange(64), rng.integers(0, 3, 64)] = rng.choice([EDGE * vs, -EDGE * vs - 1e-9, 1e30, -1e30, (EDGE - 1) * vs, -EDGE * vs], 64)
    pts.append(far)
    pts.append(extra)
    xyz = np.concatenate(pts)
    maps = sorted(set(ids[:, 0].tolist()))
    m = rng.choice(maps, len(xyz)).astype(np.int32)
    wrong = rng.random(len(xyz)) < 0.05
    m[wrong] = rng.choice([-1, -7, 1023, 1024, 1 << 20, 1, 6], int(wrong.sum()))
    assert len(xyz) == n
    return xyz, m
