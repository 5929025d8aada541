"""Fields of the mesh tests (tests/test_tsdf_mesh_ref.py on the CPU, tests/test_gpu_tsdf_mesh.py on the device), as raw blocks -- what
TsdfMap.load_blocks takes and TsdfMap.blocks() returns.  Every voxel has Sq = q + 1024 W with a random q (so num = q, zeros included: a zero counts
as not positive).  The noise fields are 3 x 3 x 3 blocks with bx, by, bz in {-2, -1, 0} (13.8 k voxels): cells across block borders in every
direction, across the coordinate origin, and at the outer boundary where the neighbour block is absent."""
import functools

import numpy as np

VOXEL_SIZE = 0.2
SEED = 20          # chosen so that all 256 configurations occur among the meshable cells of noise_full and of noise_holes (the CPU test asserts it)


def _field(rng, n, w_lo, w_hi):
    """n blocks of random voxels: W in w_lo .. w_hi, q in [-1024, 1024] with about 4 % exact zeros, Wc = W, I below 256 Wc"""
    W = rng.integers(w_lo, w_hi + 1, (n, 512))
    q = rng.integers(-1024, 1025, (n, 512))
    q[rng.random((n, 512)) < 0.04] = 0
    Wc = W.copy()
    I = rng.integers(0, 256, (n, 512)) * Wc
    return W, q, Wc, I


def _voxels(W, q, Wc, I):
    q = np.where(W == 0, np.abs(q), q)   # (Sq is unsigned: an unseen voxel keeps a non-negative sum)
    Sq = q + 1024 * W
    assert Sq.min() >= 0 and Sq.max() < 2 ** 32
    return np.stack([W, Sq, Wc, I], -1).astype(np.uint32)


def _grid_ids(map_id, lo, hi):
    r = np.arange(lo, hi)
    b = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([np.full((len(b), 1), map_id), b], 1).astype(np.int32)


def _noise_full(rng):
    ids = _grid_ids(0, -2, 1)
    return ids, _voxels(*_field(rng, len(ids), 2, 4))


def _noise_holes(rng):
    ids = _grid_ids(0, -2, 1)
    ids = ids[~(ids[:, 1:] == -1).all(1)]                  # the centre block is absent
    W, q, Wc, I = _field(rng, len(ids), 1, 3)              # min_weight = 2 changes the answer
    u = rng.random(W.shape)
    W[u < 0.10] = 0
    Wc[(u >= 0.10) & (u < 0.13)] = 0
    W[(u >= 0.13) & (u < 0.132)] = 1 << 20                  # a weight at the limit is not good
    Wc = np.where(W == 0, 0, Wc)
    I = np.where(Wc == 0, 0, np.minimum(I, 255 * Wc))
    return ids, _voxels(W, q, Wc, I)


def _two_maps(rng):
    a, b = _grid_ids(0, -1, 1), _grid_ids(5, -1, 1)
    ids = np.concatenate([a, b])
    return ids, _voxels(*_field(rng, len(ids), 1, 3))


def _sphere():
    """24^3 voxels around a sphere of radius 1.31 m whose centre lies off the lattice: D = the clamped distance to the surface, quantised as the
    integration quantises one view; only voxels within tau of the surface are seen"""
    vs = np.float64(np.float32(0.15))
    J = 3
    tau = J * vs
    kq = 1024.0 / tau
    centre = np.array([1.8317, 1.7891, 1.8043])
    ids = _grid_ids(0, 0, 3)
    l = np.arange(512)
    idx = np.stack([ids[:, 1 + a, None] * 8 + ((l >> (3 * a)) & 7)[None, :] for a in range(3)], -1)   # (n, 512, 3)
    X = (idx.astype(np.float64) + 0.5) * vs
    sdf = np.sqrt(((X - centre) ** 2).sum(-1)) - 1.31
    seen = np.abs(sdf) <= tau
    q = np.rint(np.clip(sdf, -tau, tau) * kq).astype(np.int64)
    W = seen.astype(np.int64)
    return ids, _voxels(W, np.where(seen, q, 0), W, 100 * W), float(vs), centre


def _scene():
    import tsdf_cases as TC
    return TC.reference_of("scene").dump()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(ids (n, 4) int32, voxels (n, 512, 4) uint32, voxel_size)"""
    rng = np.random.default_rng(SEED)
    out = {}
    for name, fn in (("noise_full", _noise_full), ("noise_holes", _noise_holes), ("two_maps", _two_maps)):
        ids, vox = fn(rng)
        out[name] = dict(ids=ids, voxels=vox, voxel_size=VOXEL_SIZE)
    ids, vox, vs, centre = _sphere()
    out["sphere"] = dict(ids=ids, voxels=vox, voxel_size=vs, centre=centre)
    ids, vox = _scene()
    out["scene"] = dict(ids=ids, voxels=vox, voxel_size=0.2)
    for c in out.values():
        c["ids"].setflags(write=False); c["voxels"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_of(name, min_weight=1, map_id=-1):
    """the yardstick's canonical (vertices, triangles) of a case, computed once and shared: do not change it"""
    import tsdf_mesh_ref as MR
    c = cases()[name]
    return MR.mesh(c["ids"], c["voxels"], c["voxel_size"], min_weight, map_id)
