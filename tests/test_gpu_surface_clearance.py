"""GPU: KeyframePipeline.surface_clearance() on the two-segment step of tests/test_gpu_surface_map.py (full-size frames, two segments of three)
against the yardstick tests/tsdf_distance_ref.py fed with that map's own dump: the layer's blocks, cell words and counts bit for bit, point queries,
and the costmap dense.clearance_slice cuts from it.  The radius is 1.6 m: eight voxels of 0.2 m, TsdfMap.distance's default."""
import time

import numpy as np
import pytest

import tsdf_distance_ref as DR

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=3, unique_frames=3, seed=5, ba_windows="tracks", depth="sgbm")
SEGMENTS = [3, 3]
MAP_KW = dict(voxel_size=0.2, trunc_voxels=4, log2_blocks=15)
RADIUS_M = 1.6


@pytest.fixture(scope="module")
def pipe():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(sum(SEGMENTS), segments=SEGMENTS, **KW)
    p.step()
    yield p
    p.close()


def test_surface_clearance_equals_the_yardstick(pipe):
    from stereo_visual_slam_amd.dense import clearance_slice
    tm = pipe.surface_map(**MAP_KW)
    try:
        ids, vox = tm.blocks()
        assert len(ids) > 1000 and set(ids[:, 0].tolist()) == {0, 1}, "a real map: thousands of blocks, both segments"
        got = pipe.surface_clearance(RADIUS_M)
        assert got["radius"] == 8 and got["voxel_size"] == float(np.float32(0.2))
        t0 = time.perf_counter()
        want = DR.layer(ids, vox, -1, 1, 8, MAP_KW["log2_blocks"])
        print("yardstick at R = 8: %d blocks, %d sites, %d layer blocks, %.2f s" % (len(ids), want["counts"][0], want["counts"][1], time.perf_counter() - t0))
        assert not want["void"] and want["counts"][0] > 5000 and want["counts"][2] > 0
        assert got["counts"] == want["counts"]
        assert np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["cells"], want["cells"])
        assert tm.stats()["status"] == 0
        # queries around the sites of both segments, and away from them
        rng = np.random.default_rng(2)
        vs = got["voxel_size"]
        pts, maps = [], []
        for m, s in want["sites"].items():
            pick = s[rng.integers(0, len(s), 1024)]
            pts.append((pick + rng.uniform(-10, 11, pick.shape)) * vs)
            maps.append(np.full(len(pick), m, np.int32))
        pts, maps = np.concatenate(pts), np.concatenate(maps)
        dist, cls = tm.distance_query(pts, maps)
        wd, wc = DR.query(want, pts, maps, 0.2)
        assert np.array_equal(dist.view(np.uint32), wd.view(np.uint32)) and np.array_equal(cls, wc)
        assert np.isfinite(dist).sum() > 500 and (cls == DR.FREE).any() and (cls == DR.OCCUPIED).any()
        # the costmap of segment 0 over a band around the cameras' height: as many finite columns as the layer has there
        band = clearance_slice(got["ids"], got["cells"], vs, axis=1, lo=0, hi=8, map_id=0)
        sel = (want["ids"][:, 0] == 0) & (want["ids"][:, 2] == 0)
        assert sel.any() and band["d2"].shape[0] % 8 == 0
        cols = (want["cells"][sel].reshape(-1, 8, 8, 8) & 0xFFF).min(axis=2)            # (block, z, x): the minimum over y
        assert (band["d2"] != DR.FAR).sum() == (cols != DR.FAR).sum()
        with pytest.raises(AssertionError):
            pipe.surface_clearance(3.5)     # 18 voxels
    finally:
        tm.close()
