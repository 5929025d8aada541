"""GPU: the mesh of KeyframePipeline.surface_map() -- tm.mesh() against the numpy yardstick tests/tsdf_mesh_ref.py fed tm.blocks(), and the PLY
file.  The smallest depth="sgbm" window configuration of tests/test_gpu_surface_map.py with its side tests' gates."""
import numpy as np
import pytest

import tsdf_mesh_ref as MR

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=3, unique_frames=3, seed=5, ba_windows="tracks", depth="sgbm")
SEGMENTS = [3, 3]
MAP_KW = dict(voxel_size=0.2, trunc_voxels=4, log2_blocks=15)
LEAN = dict(z_min=10.0, z_max=20.0, step=2)


@pytest.fixture(scope="module")
def surface():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(sum(SEGMENTS), segments=SEGMENTS, **KW)
    p.step()
    tm = p.surface_map(**MAP_KW, **LEAN)
    yield tm
    tm.close()
    p.close()


@pytest.mark.parametrize("min_weight", [1, 2])
def test_the_mesh_of_a_surface_map_equals_the_yardstick(surface, min_weight):
    ids, vox = surface.blocks()
    assert len(ids) > 100 and set(ids[:, 0].tolist()) == {0, 1}, "a real map: both segments"
    want_v, want_t = MR.mesh(ids, vox, MAP_KW["voxel_size"], min_weight)
    got_v, got_t = surface.mesh(min_weight=min_weight)
    assert len(want_t) > 500 and surface.last_counts == (len(want_v), len(want_t))
    assert got_v.tobytes() == want_v.tobytes() and got_v.tobytes() == surface.extract(min_weight=min_weight).tobytes()
    assert got_t.dtype == np.int32 and np.array_equal(got_t, want_t)
    one_v, one_t = surface.mesh(map_id=1, min_weight=min_weight)
    lo = int(np.searchsorted(want_v["map"], 1))
    assert one_v.tobytes() == want_v[lo:].tobytes() and np.array_equal(one_t + lo, want_t[(want_t >= lo).all(1)])


def test_write_mesh_ply_round_trip(surface, tmp_path):
    from stereo_visual_slam_amd.dense import read_mesh_ply, write_mesh_ply
    v, t = surface.mesh(min_weight=2)
    path = str(tmp_path / "surface_mesh.ply")
    write_mesh_ply(path, v, t)
    rv, rt = read_mesh_ply(path)
    assert len(rv) == len(v) > 0 and np.array_equal(rt, t)
    for name in rv.dtype.names:
        assert np.array_equal(rv[name].view(np.uint32), v[name].view(np.uint32)), name
