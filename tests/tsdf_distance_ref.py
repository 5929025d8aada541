"""The surface map's clearance layer in numpy (include/vslam_hip.h "DISTANCE"), restated from the definition and not the way the kernels compute it.

Input: a TsdfMap.blocks() dump.  Every voxel is classed with EXTRACTION's predicate, the sites are the OCCUPIED voxels with a FREE face neighbour,
and every site STAMPS its ball of integer offsets |o|^2 <= R^2 into the layer with a running minimum -- a scatter from the sites, where form 0 of the
device gathers over site masks and form 1 runs three one-dimensional passes.  The cost is sites x ball size (2109 offsets at R = 8, 17077 at R = 16).
The layer's table (slots, probing) is not restated beyond its size: a build is void when the blocks it claims before it computes anything -- the
claimed blocks of the covered maps and every in-range block within ceil(R / 8) blocks per axis of a block with a site -- outnumber 2^log2_layer_blocks.
The device can void EARLIER than that: in a table of 128 slots or more its claim gives up after 128 probes, so a table at a high load factor may void
with room left, and which build does depends on the hash.  That is not restated here; the cases keep their tables at most about half full (or, at 64
slots, let the probe cover the whole table), and a later case that fills a large table further must expect a void this file does not predict.
Queries are restated in f64."""
import numpy as np

import voxel_ref as VR

MAX_MAP = VR.MAX_MAP
MAX_W = 1 << 20
HALF = 1 << 17            # voxel indices per axis: [-2^17, 2^17)
BHALF = 1 << 14           # block coordinates per axis: [-2^14, 2^14)
FAR = 0xFFF
UNKNOWN, FREE, OCCUPIED, INVALID = 0, 1, 2, 3
VOID_BIT = 16             # vslam_tsdf_stats.status bit 4
_L = np.arange(512)
_LOCAL = np.stack([(_L >> (3 * a)) & 7 for a in range(3)], 1)     # (512, 3): the (x, y, z) of a block's voxel l


def _pack(i):
    """one sortable int64 per voxel index row (n, 3), all inside [-2^17, 2^17)"""
    i = np.asarray(i, np.int64)
    return ((i[:, 0] + HALF) << 36) | ((i[:, 1] + HALF) << 18) | (i[:, 2] + HALF)


def ball(R):
    """the integer offsets with |o|^2 <= R^2 as (n, 3) and their squared lengths"""
    r = np.arange(-R, R + 1)
    o = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    d2 = (o * o).sum(1)
    return o[d2 <= R * R], d2[d2 <= R * R]


def classes(vox, min_weight=1):
    """the class of every voxel of a dump's (n, 512, 4) sums"""
    v = np.asarray(vox, np.int64)
    good = (v[..., 0] >= max(int(min_weight), 1)) & (v[..., 0] < MAX_W) & (v[..., 2] >= 1)
    num = v[..., 1] - 1024 * v[..., 0]
    return np.where(good, np.where(num > 0, FREE, OCCUPIED), UNKNOWN).astype(np.uint8)


def sites_of(ids, cls):
    """the sites of ONE map: ids (n, 3) block coordinates, cls (n, 512) -> (s, 3) voxel indices, sorted"""
    if not len(ids):
        return np.zeros((0, 3), np.int64)
    idx = (np.asarray(ids, np.int64)[:, None, :] * 8 + _LOCAL[None, :, :]).reshape(-1, 3)
    c = cls.reshape(-1)
    key = _pack(idx)
    order = np.argsort(key)
    key, c_sorted = key[order], c[order]
    occ = np.flatnonzero(c == OCCUPIED)
    site = np.zeros(len(occ), bool)
    for a in range(3):
        for d in (-1, 1):
            j = idx[occ].copy()
            j[:, a] += d
            inr = (j[:, a] >= -HALF) & (j[:, a] < HALF)
            k = _pack(np.where(inr[:, None], j, 0))
            pos = np.minimum(np.searchsorted(key, k), len(key) - 1)
            site |= inr & (key[pos] == k) & (c_sorted[pos] == FREE)
    s = idx[occ[site]]
    return s[np.lexsort((s[:, 2], s[:, 1], s[:, 0]))]


def stamp(sites, R, dense_limit=1 << 25, chunk=1 << 22):
    """every site's ball stamped with a running minimum: (voxel indices (m, 3), d2 (m,)) of the voxels with d2 <= R^2, inside the index range.
    Two ways to keep the minimum, same result: a dense grid over the sites' bounding box where that is small (one pass per offset of the ball), a
    sort of (voxel, d2) pairs where it is not (sites at both ends of the index range)"""
    o, od2 = ball(R)
    if not len(sites):
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    lo = sites.min(0) - R
    shape = sites.max(0) + R + 1 - lo
    if int(np.prod(shape.astype(np.float64))) <= dense_limit:
        big = np.int32(1 << 30)
        grid = np.full(int(np.prod(shape)), big, np.int32)
        stride = np.array([shape[1] * shape[2], shape[2], 1], np.int64)
        flat = (sites - lo) @ stride
        for off, d in zip((o @ stride).tolist(), od2.tolist()):      # (distinct sites, one offset: distinct targets, a plain minimum is exact)
            grid[flat + off] = np.minimum(grid[flat + off], d)
        hit = np.flatnonzero(grid < big)
        idx = np.stack(np.unravel_index(hit, tuple(shape)), 1).astype(np.int64) + lo
        inr = ((idx >= -HALF) & (idx < HALF)).all(1)
        return idx[inr], grid[hit][inr].astype(np.int64)
    keys, vals = np.zeros(0, np.int64), np.zeros(0, np.int64)
    per = max(chunk // len(o), 1)
    for s0 in range(0, len(sites), per):
        t = (sites[s0:s0 + per, None, :] + o[None, :, :]).reshape(-1, 3)
        d = np.broadcast_to(od2[None, :], (len(sites[s0:s0 + per]), len(o))).reshape(-1)
        inr = ((t >= -HALF) & (t < HALF)).all(1)
        k = np.concatenate([keys, _pack(t[inr])])
        d = np.concatenate([vals, d[inr]])
        order = np.lexsort((d, k))
        k, d = k[order], d[order]
        first = np.concatenate([[True], k[1:] != k[:-1]]) if len(k) else np.zeros(0, bool)
        keys, vals = k[first], d[first]           # (sorted by key, then by d2: the first of a key is its minimum)
    idx = np.stack([(keys >> 36) - HALF, ((keys >> 18) & (2 * HALF - 1)) - HALF, (keys & (2 * HALF - 1)) - HALF], 1)
    return idx, vals


def candidates(claimed, site_blocks, R):
    """the blocks a build claims in the layer's table before it computes: the claimed ones and the in-range dilation of the site blocks"""
    rb = (R + 7) // 8
    r = np.arange(-rb, rb + 1)
    off = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    out = set(map(tuple, np.asarray(claimed, np.int64).reshape(-1, 3).tolist()))
    if len(site_blocks):
        c = (np.asarray(site_blocks, np.int64)[:, None, :] + off[None, :, :]).reshape(-1, 3)
        c = c[((c >= -BHALF) & (c < BHALF)).all(1)]
        out.update(map(tuple, np.unique(c, axis=0).tolist()))
    return out


def layer(ids, vox, map_id=-1, min_weight=1, radius=8, log2_layer_blocks=16):
    """TsdfMap.distance() of a dump: dict(ids (n, 4) int32, cells (n, 512) uint16, counts (sites, layer blocks, blocks of kind (b) only), void, status
    -- the bits the build adds to vslam_tsdf_stats.status --, sites {map: (s, 3)}), blocks sorted by (map, bx, by, bz)"""
    ids = np.asarray(ids, np.int64).reshape(-1, 4)
    vox = np.asarray(vox).reshape(len(ids), 512, 4)
    R = int(radius)
    assert 1 <= R <= 16
    cover = np.ones(len(ids), bool) if map_id < 0 else ids[:, 0] == map_id
    ids, cls = ids[cover], classes(vox[cover], min_weight)
    blocks, sites, n_cand = {}, {}, 0
    for m in sorted(set(ids[:, 0].tolist())):
        sel = ids[:, 0] == m
        s = sites_of(ids[sel, 1:], cls[sel])
        sites[m] = s
        n_cand += len(candidates(ids[sel, 1:], np.unique(s >> 3, axis=0) if len(s) else s, R))
        for b, c in zip(ids[sel, 1:].tolist(), cls[sel]):
            blocks[(m,) + tuple(b)] = (FAR | (c.astype(np.uint16) << 12)).astype(np.uint16)
        idx, d2 = stamp(s, R)
        for b in np.unique(idx >> 3, axis=0).tolist() if len(idx) else []:
            blocks.setdefault((m,) + tuple(b), np.full(512, FAR, np.uint16))
        if len(idx):
            bkey = _pack(idx >> 3)          # (block coordinates fit the voxel packing)
            order = np.argsort(bkey, kind="stable")
            cut = np.flatnonzero(np.concatenate([[True], bkey[order][1:] != bkey[order][:-1]]))
            for lo, hi in zip(cut, np.concatenate([cut[1:], [len(order)]])):
                rows = order[lo:hi]
                i = idx[rows]
                blk = blocks[(m,) + tuple((i[0] >> 3).tolist())]
                l = ((i[:, 2] & 7) << 6) | ((i[:, 1] & 7) << 3) | (i[:, 0] & 7)
                blk[l] = (blk[l] & 0xF000) | d2[rows].astype(np.uint16)
    n_sites = sum(len(s) for s in sites.values())
    if n_cand > (1 << int(log2_layer_blocks)):
        return dict(ids=np.zeros((0, 4), np.int32), cells=np.zeros((0, 512), np.uint16), counts=(n_sites, 0, 0), void=True, status=VOID_BIT, sites=sites)
    keys = sorted(blocks)
    return dict(ids=np.array(keys, np.int32).reshape(-1, 4), cells=np.stack([blocks[k] for k in keys]) if keys else np.zeros((0, 512), np.uint16),
                counts=(n_sites, len(keys), len(keys) - len(ids)), void=False, status=0, sites=sites)


def query(lay, xyz, map_id, voxel_size):
    """TsdfMap.distance_query() against a layer(): (dist (N,) float32, cls (N,) uint8)"""
    vs = np.float64(np.float32(voxel_size))
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    m = np.array(np.broadcast_to(np.asarray(map_id, np.int64), (len(xyz),)))
    with np.errstate(all="ignore"):
        i = np.floor(xyz / vs)
        valid = (m >= 0) & (m <= MAX_MAP) & np.isfinite(xyz).all(1) & ((i >= -HALF) & (i < HALF)).all(1)
    word = np.full(len(xyz), FAR, np.uint16)
    table = {tuple(k): c for k, c in zip(lay["ids"].tolist(), lay["cells"])}
    iv = np.where(valid[:, None], i, 0).astype(np.int64)
    for n in np.flatnonzero(valid):
        blk = table.get((int(m[n]),) + tuple((iv[n] >> 3).tolist()))
        if blk is not None:
            word[n] = blk[((iv[n, 2] & 7) << 6) | ((iv[n, 1] & 7) << 3) | (iv[n, 0] & 7)]
    d2, cls = (word & 0xFFF).astype(np.int64), ((word >> 12) & 3).astype(np.uint8)
    dist = (np.sqrt(d2.astype(np.float64)) * vs).astype(np.float32)
    dist = np.where((cls == OCCUPIED) & (d2 > 0), -dist, dist)
    dist = np.where(d2 == FAR, np.where(cls == OCCUPIED, -np.inf, np.inf), dist).astype(np.float32)
    dist[~valid] = np.inf
    cls[~valid] = INVALID
    return dist, cls
