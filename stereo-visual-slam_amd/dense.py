"""The map stages on the host: a voxel list (VoxelMap.extract()) or a surfel list (TsdfMap.extract()) to and from a PLY file.  Pure numpy."""
import numpy as np

_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("count", "<u4")])
_PLY_TYPES = {"<f4": "float", "<u4": "uint"}


def write_ply(path, voxels):
    """voxels (a structured array with x, y, z, intensity, count: VoxelMap.extract()) -> a binary little-endian PLY of one vertex per voxel"""
    v = np.zeros(len(voxels), _PLY_DTYPE)
    for name in _PLY_DTYPE.names:
        v[name] = voxels[name]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
    head += ["property %s %s" % (_PLY_TYPES[_PLY_DTYPE[name].str], name) for name in _PLY_DTYPE.names]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(v.tobytes())


def read_ply(path):
    """the vertices of a file write_ply wrote, as a structured array (x, y, z, intensity, count)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"], head[:2]
    n = int(next(ln for ln in head if ln.startswith("element vertex")).split()[2])
    props = [tuple(ln.split()[1:]) for ln in head if ln.startswith("property")]
    assert props == [(_PLY_TYPES[_PLY_DTYPE[name].str], name) for name in _PLY_DTYPE.names], props
    return np.frombuffer(data[end:], _PLY_DTYPE, count=n).copy()


# ---- the surface map's surfels (TsdfMap.extract()): the same file layout with a normal per vertex
_SURFEL_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("intensity", "<f4"), ("weight", "<u4")])


def write_surfel_ply(path, surfels):
    """surfels (a structured array with x, y, z, nx, ny, nz, intensity, weight: TsdfMap.extract()) -> a binary little-endian PLY of one oriented
    vertex per surfel"""
    v = np.zeros(len(surfels), _SURFEL_PLY_DTYPE)
    for name in _SURFEL_PLY_DTYPE.names:
        v[name] = surfels[name]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
    head += ["property %s %s" % (_PLY_TYPES[_SURFEL_PLY_DTYPE[name].str], name) for name in _SURFEL_PLY_DTYPE.names]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(v.tobytes())


def read_surfel_ply(path):
    """the vertices of a file write_surfel_ply wrote, as a structured array (x, y, z, nx, ny, nz, intensity, weight)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"], head[:2]
    n = int(next(ln for ln in head if ln.startswith("element vertex")).split()[2])
    props = [tuple(ln.split()[1:]) for ln in head if ln.startswith("property")]
    assert props == [(_PLY_TYPES[_SURFEL_PLY_DTYPE[name].str], name) for name in _SURFEL_PLY_DTYPE.names], props
    return np.frombuffer(data[end:], _SURFEL_PLY_DTYPE, count=n).copy()


_FACE_PLY_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_mesh_ply(path, vertices, triangles):
    """(vertices, triangles) of TsdfMap.mesh() -> a binary little-endian PLY: the vertex properties of write_surfel_ply, then one face per triangle
    (`property list uchar int vertex_indices`, corner order kept: counter-clockwise seen from free space)"""
    triangles = np.asarray(triangles, np.int32).reshape(-1, 3)
    assert len(triangles) == 0 or (triangles.min() >= 0 and triangles.max() < len(vertices)), "triangle indices outside the vertex array"
    v = np.zeros(len(vertices), _SURFEL_PLY_DTYPE)
    for name in _SURFEL_PLY_DTYPE.names:
        v[name] = vertices[name]
    f3 = np.zeros(len(triangles), _FACE_PLY_DTYPE)
    f3["n"] = 3
    f3["v"] = triangles
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
    head += ["property %s %s" % (_PLY_TYPES[_SURFEL_PLY_DTYPE[name].str], name) for name in _SURFEL_PLY_DTYPE.names]
    head += ["element face %d" % len(f3), "property list uchar int vertex_indices"]
    with open(path, "wb") as f:
        f.write(("\n".join(head + ["end_header"]) + "\n").encode("ascii"))
        f.write(v.tobytes())
        f.write(f3.tobytes())


def read_mesh_ply(path):
    """(vertices, triangles) of a file write_mesh_ply wrote: a structured array (x, y, z, nx, ny, nz, intensity, weight) and (n, 3) int32"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"], head[:2]
    n = int(next(ln for ln in head if ln.startswith("element vertex")).split()[2])
    nf = int(next(ln for ln in head if ln.startswith("element face")).split()[2])
    props = [tuple(ln.split()[1:]) for ln in head if ln.startswith("property")]
    assert props == [(_PLY_TYPES[_SURFEL_PLY_DTYPE[name].str], name) for name in _SURFEL_PLY_DTYPE.names] + [("list", "uchar", "int", "vertex_indices")], props
    v = np.frombuffer(data[end:], _SURFEL_PLY_DTYPE, count=n).copy()
    f3 = np.frombuffer(data[end + v.nbytes:], _FACE_PLY_DTYPE, count=nf)
    assert (f3["n"] == 3).all()
    return v, f3["v"].astype(np.int32)


def write_depth_pgm(path, depth, z_max):
    """one depth view of TsdfMap.render() (h, w) -> a binary 16-bit PGM any image viewer opens: 0 = the ray missed, otherwise
    1 .. 65535 = round(depth / z_max * 65535) (a hit nearer than z_max / 65535 / 2 is stored as 1, one beyond z_max as 65535)"""
    depth = np.asarray(depth, np.float64)
    assert depth.ndim == 2 and z_max > 0, (depth.shape, z_max)
    v = np.where(depth > 0, np.clip(np.rint(depth / z_max * 65535.0), 1, 65535), 0).astype(">u2")
    with open(path, "wb") as f:
        f.write(("P5\n%d %d\n65535\n" % (depth.shape[1], depth.shape[0])).encode("ascii"))
        f.write(v.tobytes())


def clearance_slice(ids, cells, voxel_size, axis=1, lo=0, hi=1, map_id=None):
    """The costmap a ground planner reads off a clearance layer (TsdfMap.distance: ids (n, 4) of (map, bx, by, bz), cells (n, 512) uint16): over the
    voxel indices [lo, hi) along `axis`, per column of the other two axes the minimum squared distance d2 (voxel units; 0xFFF where every voxel of
    the column is FAR or outside the layer) and whether any voxel of the column is OCCUPIED.  map_id: the map to read (None: every block given).
    Returns dict(d2 (na, nb) uint16, occupied (na, nb) bool, origin (ia, ib) -- the voxel indices of d2[0, 0] along the two remaining axes in
    ascending axis order, so the column's corner in metres is origin * voxel_size --, axes (a, b), voxel_size); empty (0, 0) arrays when no block
    meets the band."""
    ids = np.asarray(ids, np.int64).reshape(-1, 4)
    cells = np.asarray(cells, np.uint16).reshape(len(ids), 8, 8, 8)   # (z, y, x)
    assert axis in (0, 1, 2) and hi > lo, (axis, lo, hi)
    a, b = [k for k in range(3) if k != axis]
    keep = (ids[:, 1 + axis] * 8 + 7 >= lo) & (ids[:, 1 + axis] * 8 < hi)
    if map_id is not None:
        keep &= ids[:, 0] == map_id
    ids, cells = ids[keep], cells[keep]
    if not len(ids):
        return dict(d2=np.zeros((0, 0), np.uint16), occupied=np.zeros((0, 0), bool), origin=(0, 0), axes=(a, b), voxel_size=float(voxel_size))
    a0, b0 = int(ids[:, 1 + a].min()) * 8, int(ids[:, 1 + b].min()) * 8
    na, nb = int(ids[:, 1 + a].max()) * 8 + 8 - a0, int(ids[:, 1 + b].max()) * 8 + 8 - b0
    d2 = np.full((na, nb), 0xFFF, np.uint16)
    occ = np.zeros((na, nb), bool)
    for bid, blk in zip(ids, cells):
        blk = np.moveaxis(blk.transpose(2, 1, 0), axis, 2)           # (x, y, z) -> (a, b, axis)
        k = np.arange(8) + bid[1 + axis] * 8
        blk = blk[:, :, (k >= lo) & (k < hi)]
        ia, ib = int(bid[1 + a]) * 8 - a0, int(bid[1 + b]) * 8 - b0
        d2[ia:ia + 8, ib:ib + 8] = np.minimum(d2[ia:ia + 8, ib:ib + 8], (blk & 0xFFF).min(axis=2))
        occ[ia:ia + 8, ib:ib + 8] |= (((blk >> 12) & 3) == 2).any(axis=2)
    return dict(d2=d2, occupied=occ, origin=(a0, b0), axes=(a, b), voxel_size=float(voxel_size))


def read_depth_pgm(path, z_max):
    """the (h, w) float64 depth of a file write_depth_pgm wrote with the same z_max: 0 where the ray missed, otherwise within z_max / 131070 of the
    depth written"""
    with open(path, "rb") as f:
        data = f.read()
    magic, size, peak, rest = data.split(b"\n", 3)
    assert magic == b"P5" and peak == b"65535", (magic, peak)
    w, h = (int(s) for s in size.split())
    return np.frombuffer(rest, ">u2", count=w * h).reshape(h, w).astype(np.float64) * (z_max / 65535.0)
