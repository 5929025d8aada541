"""GPU: KeyframePipeline.surface_views() -- the surface map of a step seen again from every frame of dense_map_inputs() at a quarter of the image
size -- against the numpy yardstick tests/tsdf_render_ref.py over the blocks the map holds, bit for bit; the fused disparity; the PGM file."""
import numpy as np
import pytest

import tsdf_render_ref as RR

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=2, unique_frames=2, seed=5, ba_windows="tracks", depth="sgbm")
MAP_KW = dict(voxel_size=0.2, trunc_voxels=4, log2_blocks=15, step=2)


@pytest.fixture(scope="module")
def pipe():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(2, **KW)
    p.step()
    yield p
    p.close()


@pytest.fixture(scope="module")
def views(pipe):
    tm = pipe.surface_map(**MAP_KW)
    out = pipe.surface_views(scale=0.25, disparity=True)
    yield tm, out
    tm.close()


def test_surface_views_equal_the_yardstick_over_the_maps_blocks(pipe, views):
    tm, out = views
    p = pipe.vo.params
    T, map_id = pipe.dense_map_inputs()
    assert np.array_equal(out["T_c_w"], T) and np.array_equal(out["map_id"], map_id) and map_id.tolist() == [0, 0]
    w, h = int(round(pipe.w * 0.25)), int(round(pipe.h * 0.25))
    K4 = tuple(float(v) * 0.25 for v in p.cam[:4])
    assert out["depth"].shape == (2, h, w) and out["normal"].shape == (2, h, w, 3) and out["intensity"].shape == (2, h, w) and out["K4"] == K4
    ids, vox = tm.blocks()
    want = RR.render(ids, vox, tm.voxel_size, T, map_id, K4, (w, h), p.depth_min, p.depth_reliable, 0.5, 1)
    print("surface views: %d blocks, %d of %d rays hit, K %d, margins D %.3g g %.3g" % (len(ids), want["hits"], 2 * h * w, want["K"], want["margin_D"], want["margin_g"]))
    assert want["hits"] > 1000, "a real view: more than a thousand rays hit"
    attr = np.concatenate([out["normal"], out["intensity"][..., None]], -1)
    assert np.array_equal(out["depth"].view(np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(attr.view(np.uint32), want["attr"].view(np.uint32))
    assert out["counts"][0] == want["hits"]
    # tsdf_map= names the map, min_weight and march reach the call
    other = pipe.surface_views(tsdf_map=tm, scale=0.25, march=1.0, min_weight=2)
    direct = tm.render(T, map_id, K4=K4, size=(w, h), march=1.0, min_weight=2)   # (held to the yardstick by tests/test_gpu_tsdf_render.py)
    assert other["depth"].tobytes() == direct["depth"].tobytes() != out["depth"].tobytes() and "disparity" not in other


def test_the_fused_disparity(pipe, views):
    _, out = views
    fx, b = float(pipe.vo.params.cam[0]) * 0.25, float(pipe.vo.params.cam[4])
    hit = out["depth"] > 0
    assert hit.any() and not hit.all()
    assert out["disparity"].dtype == np.float32 and not out["disparity"][~hit].any()
    assert np.array_equal(out["disparity"][hit], (fx * b / out["depth"][hit].astype(np.float64)).astype(np.float32))


def test_write_depth_pgm_round_trips(views, tmp_path):
    from stereo_visual_slam_amd.dense import read_depth_pgm, write_depth_pgm
    _, out = views
    depth, z_max = out["depth"][0], 40.0
    path = str(tmp_path / "view.pgm")
    write_depth_pgm(path, depth, z_max)
    with open(path, "rb") as f:
        assert f.read(2) == b"P5"
    back = read_depth_pgm(path, z_max)
    assert back.shape == depth.shape and np.array_equal(back == 0, depth == 0)
    assert np.abs(back - depth).max() <= z_max / 65535.0 / 2 * 1.0001
