"""The numpy restatement of the dense map stage (tests/voxel_ref.py) on cases worked by hand: it is the yardstick of tests/test_gpu_voxel.py,
so its own arithmetic is pinned here, without a GPU.  Voxel size 0.5 keeps the hand arithmetic exact (inv = 2.0f)."""
import numpy as np

import voxel_ref as VR


def _one(ref):
    v = ref.extract()
    assert len(v) == 1
    return v[0]


def test_negative_coordinates_floor_not_truncate():
    ref = VR.VoxelRef(0.5)
    ref.insert([[-0.25, -0.75, -1.0]])        # t = -0.5, -1.5, -2.0 -> cells -1, -2, -2 (truncation would say 0, -1, -2)
    v = _one(ref)
    assert (v["ix"], v["iy"], v["iz"], v["count"]) == (-1, -2, -2, 1)
    # offsets 128, 128, 0 -> centroid (cell + (o + 0.5) / 256) * 0.5
    assert v["x"] == np.float32((-1 + 128.5 / 256) * 0.5) and v["y"] == np.float32((-2 + 128.5 / 256) * 0.5) and v["z"] == np.float32((-2 + 0.5 / 256) * 0.5)


def test_point_on_a_voxel_face_belongs_to_the_upper_voxel():
    ref = VR.VoxelRef(0.5)
    ref.insert([[1.0, 0.0, -0.5]])            # t = 2.0, 0.0, -1.0: on a face on every axis
    v = _one(ref)
    assert (v["ix"], v["iy"], v["iz"]) == (2, 0, -1)
    ok, i, o = VR.axis_key(np.float32([1.0, 0.0, -0.5]), VR.voxel_scale(0.5)[1])
    assert ok.all() and o.tolist() == [0, 0, 0]


def test_tiny_negative_coordinate_saturates_the_offset():
    ok, i, o = VR.axis_key(np.float32([-1e-10]), VR.voxel_scale(0.5)[1])   # t - floor(t) rounds to 1.0f: 256 -> 255
    assert ok.all() and i.tolist() == [-1] and o.tolist() == [255]


def test_range_drop_and_non_finite():
    ref = VR.VoxelRef(0.5)
    pts = np.float32([[65536.0, 0, 0],        # t = 2^17: first cell outside
                      [-65536.0, 0, 0],       # t = -2^17: the last cell inside
                      [-65536.25, 0, 0],      # floor = -2^17 - 1: outside
                      [0, np.nan, 0], [0, 0, np.inf], [0, -np.inf, 0],
                      [0.25, 0.25, 0.25]])
    ref.insert(pts)
    assert ref.n_dropped_range == 5 and ref.n_points == 2 and ref.n_offered == 7
    v = ref.extract()
    assert v["ix"].tolist() == [-VR.HALF, 0] and v["count"].tolist() == [1, 1]


def test_two_maps_with_equal_coordinates_stay_apart():
    ref = VR.VoxelRef(0.5)
    p = [[0.25, 0.25, 0.25]]
    ref.insert(p, map_id=0); ref.insert(p, map_id=VR.MAX_MAP); ref.insert(p, map_id=VR.MAX_MAP)
    v = ref.extract()
    assert v["map"].tolist() == [0, VR.MAX_MAP] and v["count"].tolist() == [1, 2]
    assert len(ref.extract(map_id=VR.MAX_MAP)) == 1 and len(ref.extract(map_id=5)) == 0
    assert ref.extract(min_count=2)["map"].tolist() == [VR.MAX_MAP]
    assert int(ref.keys.max()) != 2 ** 64 - 1   # all-ones stays the empty slot


def test_sums_centroid_intensity_and_the_valid_mask():
    ref = VR.VoxelRef(0.5)
    pts = np.float32([[0.25, 0.0, 0.0], [0.375, 0.0, 0.0], [0.3, 0.0, 0.0]])
    ref.insert(pts, valid=[1, 1, 0], intensity=[10, 21, 200])     # the third point is masked out
    assert ref.sums.tolist() == [[2, 128 + 192, 0, 0, 31]]
    v = _one(ref)
    assert v["x"] == np.float32((160.5 / 256) * 0.5) and v["y"] == np.float32((0.5 / 256) * 0.5) and v["intensity"] == np.float32(15.5)
    # two inserts in a row equal one insert of both lists, whatever the order
    a = VR.VoxelRef(0.5); a.insert(pts[:1], intensity=[10]); a.insert(pts[1:2], intensity=[21])
    b = VR.VoxelRef(0.5); b.insert(pts[1::-1], intensity=[21, 10])
    assert np.array_equal(a.extract(), v.reshape(1)) and np.array_equal(b.extract(), v.reshape(1))


def test_scale_is_float32():
    vs, inv = VR.voxel_scale(0.2)
    assert vs.dtype == np.float32 and inv.dtype == np.float32 and inv == np.float32(1.0) / np.float32(0.2)
    ok, i, o = VR.axis_key(np.float32([0.6]), inv)    # 0.6f * inv in float32, not 3.0 in real arithmetic
    t = np.float32(0.6) * inv
    assert i.tolist() == [int(np.floor(t))] and o.tolist() == [int((t - np.floor(t)) * np.float32(256))]
