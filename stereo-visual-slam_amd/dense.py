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
