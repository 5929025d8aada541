"""The dense map stage in numpy (include/vslam_hip.h "dense map"): key, accumulation and extraction of the voxel table, restated exactly.

Every f32 product and difference is a numpy float32 operation (IEEE, rounded once, no contraction), the sums are integers, the centroids
are float64 arithmetic in the header's order cast to float32: the device kernels must give these bits, whatever order their points arrive in.
The table itself (slots, probing, capacity) is not restated: a table that never fills holds exactly these voxels."""
import numpy as np

HALF = 1 << 17          # voxel indices per axis: [-2^17, 2^17)
MAX_MAP = 1022
VOXEL_MAP_DTYPE = np.dtype([("map", "<i4"), ("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("count", "<u4"),
                            ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])


def voxel_scale(voxel_size):
    """(vs, inv) as the table stores them: vs = (float)voxel_size, inv = 1.0f / vs"""
    vs = np.float32(voxel_size)
    return vs, np.float32(1.0) / vs


def axis_key(x, inv):
    """one axis: (in range, cell index i, offset o in 1/256 voxel) of float32 coordinates x"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * inv                                   # float32 * float32 -> float32, rounded once
        c = np.floor(t)
        ok = np.isfinite(t) & (c >= -HALF) & (c < HALF)
        o = np.where(ok, (t - c) * np.float32(256.0), np.float32(0)).astype(np.int64)
    i = np.where(ok, c, 0).astype(np.int64)
    return ok, i, np.minimum(o, 255)


def pack_key(map_id, ix, iy, iz):
    return (np.uint64(map_id) << np.uint64(54)) | ((ix + HALF).astype(np.uint64) << np.uint64(36)) | ((iy + HALF).astype(np.uint64) << np.uint64(18)) | \
        (iz + HALF).astype(np.uint64)


def unpack_key(key):
    m = (key >> np.uint64(54)).astype(np.int64)
    f = lambda s: ((key >> np.uint64(s)) & np.uint64(0x3FFFF)).astype(np.int64) - HALF
    return m, f(36), f(18), f(0)


class VoxelRef:
    """a voxel map as a sorted key array and its five integer sums (count, sum_ox, sum_oy, sum_oz, sum_intensity)"""

    def __init__(self, voxel_size):
        self.vs, self.inv = voxel_scale(voxel_size)
        self.keys = np.zeros(0, np.uint64)
        self.sums = np.zeros((0, 5), np.int64)
        self.n_points = 0
        self.n_dropped_range = 0
        self.n_offered = 0      # valid points handed to insert()

    def insert(self, xyz, valid=None, intensity=None, map_id=0):
        assert 0 <= map_id <= MAX_MAP
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        keep = np.ones(len(xyz), bool) if valid is None else np.asarray(valid).reshape(-1) != 0
        g = np.zeros(len(xyz), np.int64) if intensity is None else np.asarray(intensity, np.uint8).reshape(-1).astype(np.int64)
        xyz, g = xyz[keep], g[keep]
        self.n_offered += len(xyz)
        okx, ix, ox = axis_key(xyz[:, 0], self.inv)
        oky, iy, oy = axis_key(xyz[:, 1], self.inv)
        okz, iz, oz = axis_key(xyz[:, 2], self.inv)
        ok = okx & oky & okz
        self.n_dropped_range += int((~ok).sum())
        self.n_points += int(ok.sum())
        key = pack_key(map_id, ix[ok], iy[ok], iz[ok])
        add = np.stack([np.ones(int(ok.sum()), np.int64), ox[ok], oy[ok], oz[ok], g[ok]], 1)
        keys, inv_idx = np.unique(np.concatenate([self.keys, key]), return_inverse=True)
        sums = np.zeros((len(keys), 5), np.int64)
        np.add.at(sums, inv_idx, np.concatenate([self.sums, add]))
        self.keys, self.sums = keys, sums

    def extract(self, map_id=-1, min_count=1):
        """the voxels with count >= min_count of map map_id (-1: all), sorted by (map, ix, iy, iz)"""
        m, ix, iy, iz = unpack_key(self.keys)
        n = self.sums[:, 0]
        take = (n >= max(min_count, 1)) & ((m == map_id) | (map_id < 0))
        out = np.zeros(int(take.sum()), VOXEL_MAP_DTYPE)
        out["map"], out["ix"], out["iy"], out["iz"], out["count"] = m[take], ix[take], iy[take], iz[take], n[take]
        cnt = n[take].astype(np.float64)
        vs = np.float64(self.vs)
        for name, idx, col in (("x", ix, 1), ("y", iy, 2), ("z", iz, 3)):
            out[name] = ((idx[take].astype(np.float64) + (self.sums[take, col].astype(np.float64) / cnt + 0.5) / 256.0) * vs).astype(np.float32)
        out["intensity"] = (self.sums[take, 4].astype(np.float64) / cnt).astype(np.float32)
        return out[np.lexsort((out["iz"], out["iy"], out["ix"], out["map"]))]
