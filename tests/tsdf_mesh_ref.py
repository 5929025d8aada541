"""The surface map's triangle mesh in numpy (include/vslam_hip.h "MESH"): from raw blocks to the canonical (vertices, triangles).

The vertices come through tsdf_ref.TsdfRef.extract, unchanged.  The connectivity is the header's rule restated here on its own, geometrically -- real
midpoints, real cross products, the six faces one by one -- and NOT by importing tools/gen_mc_table.py (which works in doubled integers): the
committed table csrc/mc_table.inc is held to these 256 rows by tests/test_tsdf_mesh_ref.py.  Applying the rows to a field is vectorised over all
cells of a map at once; the only Python loops run over the 256 configurations, the maps and the 15 corner slots of a row."""
import functools

import numpy as np

import tsdf_ref as TR
import voxel_ref as VR

MAX_TRIS = 5

# ------------------------------------------------------------------------------------------------------------------------ the rule
_CORNER = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], np.float64)


def _edge(k):
    """(corner a, corner b) of cube edge k = 4 e + p + 2 q: from p f^ + q g^ along e^"""
    e, p, q = k >> 2, k & 1, (k >> 1) & 1
    a = np.zeros(3, int)
    a[(e + 1) % 3], a[(e + 2) % 3] = p, q
    b = a.copy()
    b[e] = 1
    return int(a @ [1, 2, 4]), int(b @ [1, 2, 4])


EDGE_CORNERS = np.array([_edge(k) for k in range(12)])
_MID = (_CORNER[EDGE_CORNERS[:, 0]] + _CORNER[EDGE_CORNERS[:, 1]]) / 2


def _face_segments(axis, side, sign):
    """the directed segments on one face from its own four signs"""
    normal = np.zeros(3)
    normal[axis] = 1.0 if side else -1.0
    on_face = lambda c: _CORNER[c, axis] == side
    edges = [k for k in range(12) if on_face(EDGE_CORNERS[k, 0]) and on_face(EDGE_CORNERS[k, 1])]
    crossing = [k for k in edges if sign[EDGE_CORNERS[k, 0]] != sign[EDGE_CORNERS[k, 1]]]
    positive = [c for c in range(8) if on_face(c) and sign[c]]

    def directed(a, b, P):
        w = normal @ np.cross(_MID[b] - _MID[a], _CORNER[P] - _MID[a])
        assert abs(w) > 1e-9
        return (a, b) if w > 0 else (b, a)

    if len(crossing) == 2:
        return [directed(crossing[0], crossing[1], positive[0])]
    if len(crossing) == 4:
        out = []
        for P in positive:   # each positive corner is cut off by the segment between the two face edges that meet at it
            a, b = [k for k in crossing if P in EDGE_CORNERS[k]]
            out.append(directed(a, b, P))
        return out
    assert not crossing
    return []


def _same_face(a, b):
    pa, pb = _CORNER[EDGE_CORNERS[a]], _CORNER[EDGE_CORNERS[b]]
    return any((pa[:, d] == s).all() and (pb[:, d] == s).all() for d in range(3) for s in (0.0, 1.0))


def _row(cube):
    sign = [(cube >> c) & 1 for c in range(8)]
    succ = {}
    for axis in range(3):
        for side in (0, 1):
            for a, b in _face_segments(axis, side, sign):
                assert a not in succ
                succ[a] = b
    tris, left, longest = [], set(succ), 0
    while left:
        start = min(left)                        # loops in the order of their smallest member
        loop = [start]
        while succ[loop[-1]] != start:
            loop.append(succ[loop[-1]])
        left -= set(loop)
        n = len(loop)
        longest = max(longest, n)
        ok = [i for i in range(n) if not any(_same_face(loop[i], loop[(i + j) % n]) for j in range(2, n - 1))]
        i0 = min(ok, key=lambda i: loop[i])    # (raises if no such start exists)
        loop = loop[i0:] + loop[:i0]
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, n - 1)]
    return tris, longest


@functools.lru_cache(maxsize=None)
def mc_rows():
    """(count (256,), edges (256, 5, 3) int, -1 where a row has fewer triangles, longest loop)"""
    count = np.zeros(256, np.int64)
    edges = np.full((256, MAX_TRIS, 3), -1, np.int64)
    longest = 0
    for cube in range(256):
        tris, ln = _row(cube)
        count[cube] = len(tris)
        if tris:
            edges[cube, :len(tris)] = tris
        longest = max(longest, ln)
    return count, edges, longest


# ------------------------------------------------------------------------------------------------------------------------ the field
def _pack(ix, iy, iz):
    return ((ix + VR.HALF) << 36) | ((iy + VR.HALF) << 18) | (iz + VR.HALF)


def cells_of(ids, voxels, min_weight=1):
    """every cell whose lowest corner is a voxel of a listed block (one map): (ix, iy, iz, meshable, cube)"""
    ids = np.asarray(ids, np.int64).reshape(-1, 4)
    vox = np.asarray(voxels).astype(np.int64).reshape(-1, 4)
    l = np.arange(512)
    ix, iy, iz = ((ids[:, 1 + a, None] * 8 + ((l >> (3 * a)) & 7)[None, :]).ravel() for a in range(3))
    key = _pack(ix, iy, iz)
    order = np.argsort(key)
    skey, svox = key[order], vox[order]
    meshable = np.ones(len(ix), bool)
    cube = np.zeros(len(ix), np.int64)
    for c in range(8):
        jx, jy, jz = ix + (c & 1), iy + ((c >> 1) & 1), iz + ((c >> 2) & 1)
        inr = (jx < VR.HALF) & (jy < VR.HALF) & (jz < VR.HALF)
        k = _pack(jx, jy, jz)
        pos = np.minimum(np.searchsorted(skey, k), len(skey) - 1)
        hit = inr & (skey[pos] == k)
        v = svox[pos]
        good = hit & (v[:, 0] >= max(int(min_weight), 1)) & (v[:, 0] < TR.MAX_W) & (v[:, 2] >= 1)
        meshable &= good
        cube |= ((v[:, 1] - 1024 * v[:, 0] > 0) & hit).astype(np.int64) << c
    return ix, iy, iz, meshable, cube


def _vertex_key(ix, iy, iz, axis):
    return ((ix + VR.HALF) << 38) | ((iy + VR.HALF) << 20) | ((iz + VR.HALF) << 2) | axis


def triangle_keys(ids, voxels, min_weight=1):
    """the triangles of one map as vertex keys: (n, 3, 4) int64 of (ix, iy, iz, axis) per corner, in the order the rule emits them per cell"""
    count, edges, _ = mc_rows()
    ix, iy, iz, meshable, cube = cells_of(ids, voxels, min_weight)
    sel = np.flatnonzero(meshable & (count[cube] > 0))
    out = []
    for j in range(MAX_TRIS):
        s = sel[count[cube[sel]] > j]
        k = edges[cube[s], j]                                  # (n, 3) cube edges
        e, p, q = k >> 2, k & 1, (k >> 1) & 1
        base = np.stack([ix[s], iy[s], iz[s]], 1)[:, None, :].repeat(3, 1)   # (n, 3 corners, 3 axes)
        f, g = (e + 1) % 3, (e + 2) % 3
        np.put_along_axis(base, f[..., None], np.take_along_axis(base, f[..., None], 2) + p[..., None], 2)
        np.put_along_axis(base, g[..., None], np.take_along_axis(base, g[..., None], 2) + q[..., None], 2)
        out.append(np.concatenate([base, e[..., None]], 2))
    return np.concatenate(out) if out else np.zeros((0, 3, 4), np.int64)


def mesh(ids, voxels, voxel_size, min_weight=1, map_id=-1):
    """the canonical mesh of raw blocks (TsdfMap.blocks()): vertices (SURFEL_MAP_DTYPE, sorted by (map, ix, iy, iz, axis)) and triangles ((n, 3) int32
    indices into them, corner order as emitted, rows sorted lexicographically)"""
    ids = np.asarray(ids, np.int64).reshape(-1, 4)
    voxels = np.asarray(voxels).reshape(-1, 512, 4)
    ref = TR.TsdfRef(voxel_size, 1, (1.0, 1.0, 0.0, 0.0, 1.0))
    ref.blocks = {tuple(k): v.astype(np.int64) for k, v in zip(ids.tolist(), voxels)}
    verts = ref.extract(map_id, min_weight)
    tris = []
    for m in sorted(set(ids[:, 0].tolist())):
        if map_id >= 0 and m != map_id:
            continue
        tk = triangle_keys(ids[ids[:, 0] == m], voxels[ids[:, 0] == m], min_weight)
        lo, hi = np.searchsorted(verts["map"], m), np.searchsorted(verts["map"], m, side="right")
        vm = verts[lo:hi]
        vkey = _vertex_key(vm["ix"].astype(np.int64), vm["iy"].astype(np.int64), vm["iz"].astype(np.int64), vm["axis"].astype(np.int64))
        assert (np.diff(vkey) > 0).all()
        want = _vertex_key(tk[..., 0], tk[..., 1], tk[..., 2], tk[..., 3])
        pos = np.searchsorted(vkey, want)
        assert want.size == 0 or (vkey[np.minimum(pos, len(vkey) - 1)] == want).all(), "a triangle corner that is no extracted surfel"
        tris.append((pos + lo).astype(np.int32))
    tris = np.concatenate(tris) if tris else np.zeros((0, 3), np.int32)
    return verts, tris[np.lexsort((tris[:, 2], tris[:, 1], tris[:, 0]))]
