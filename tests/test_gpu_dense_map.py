"""GPU: KeyframePipeline.dense_map() -- the SGBM disparities and left images of a step fused into a voxel map at the BA-refined poses of
trajectories() -- against the numpy restatement tests/voxel_ref.py fed with the downloaded disparities, images and poses (the points come from
vslam_reproject_dev, which tests/test_gpu_voxel.py holds against the oracle); per segment against the pipeline of that segment alone; the PLY file."""
import numpy as np
import pytest

import voxel_ref as VR

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=3, unique_frames=3, seed=5, ba_windows="tracks", depth="sgbm")   # the smallest depth="sgbm" window configuration of the suite
SEGMENTS = [3, 3]
MAP_KW = dict(voxel_size=0.2, log2_capacity=20)


def _same(got, want, fields=None):
    assert len(got) == len(want), (len(got), len(want))
    for f in fields or want.dtype.names:
        bad = np.flatnonzero(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert len(bad) == 0, (f, len(bad), got[bad[:3]], want[bad[:3]])


@pytest.fixture(scope="module")
def pipe():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(sum(SEGMENTS), segments=SEGMENTS, **KW)
    p.step()
    yield p
    p.close()


def _restatement(p, T, map_id, voxel_size, z_min, z_max):
    """the voxel list the numpy restatement gives for the step p ran: reproject_dev's points of every frame with a map id, its left image as intensity"""
    import torch
    B, w, h = p.B, p.w, p.h
    with torch.cuda.stream(p.stream):
        d_T = torch.from_numpy(T).to(p.dev)
        d_xyz = torch.zeros((B, h, w, 3), dtype=torch.float32, device=p.dev); d_valid = torch.zeros((B, h, w), dtype=torch.uint8, device=p.dev)
    p.vo.reproject_dev(p.d_disp.data_ptr(), w, h, B, d_T.data_ptr(), z_min, z_max, 1, d_xyz.data_ptr(), d_valid.data_ptr())
    p.vo.sync()
    xyz, valid = d_xyz.cpu().numpy(), d_valid.cpu().numpy()
    ref = VR.VoxelRef(voxel_size)
    for b in range(B):
        if map_id[b] >= 0:
            ref.insert(xyz[b].reshape(-1, 3), valid[b].ravel(), p.h_imgs[b, :, :w].ravel(), int(map_id[b]))
    return ref


def test_dense_map_equals_the_restatement(pipe):
    p = pipe
    trajs = p.trajectories()
    T, map_id = p.dense_map_inputs()
    assert map_id.tolist() == [0, 0, 0, 1, 1, 1], "every frame of both segments is in a trajectory"
    for s, (ids, Ts) in enumerate(trajs):
        assert np.array_equal(T[p.seg_first[s] + ids], Ts)
    z_min, z_max = p.vo.params.depth_min, p.vo.params.depth_reliable
    ref = _restatement(p, T, map_id, 0.2, z_min, z_max)
    want = ref.extract()
    assert len(want) > 5000 and want["count"].max() > 50 and set(want["map"]) == {0, 1}, "a real map: many voxels, shared by many pixels"
    vm = p.dense_map(**MAP_KW)
    try:
        got = vm.extract()
        _same(got, want)
        st = vm.stats()
        assert st == dict(n_occupied=len(want), n_points=ref.n_points, n_dropped_range=ref.n_dropped_range, n_dropped_full=0, status=0), st
        # voxel_map=: a second step's points accumulate -- every sum doubles, so the centroids keep their bits
        assert p.dense_map(voxel_map=vm) is vm
        twice = vm.extract()
        assert np.array_equal(twice["count"], 2 * want["count"])
        _same(twice, want, fields=("map", "ix", "iy", "iz", "x", "y", "z", "intensity"))
    finally:
        vm.close()


def test_frames_outside_the_trajectory_contribute_nothing(pipe, monkeypatch):
    p = pipe
    T, map_id = p.dense_map_inputs()
    map_id[4] = -1                                    # as if frame 4 were in no trajectory (a frame the keyframe gate rejected)
    monkeypatch.setattr(p, "dense_map_inputs", lambda: (T, map_id))
    vm = p.dense_map(z_min=8.0, z_max=30.0, **MAP_KW)    # (a caller's own gate, too)
    try:
        _same(vm.extract(), _restatement(p, T, map_id, 0.2, 8.0, 30.0).extract())
    finally:
        vm.close()


def test_every_segment_equals_its_pipeline_alone(pipe):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    vm = pipe.dense_map(**MAP_KW)
    try:
        for s, n in enumerate(SEGMENTS):
            solo = KeyframePipeline(n, sequence=pipe.h_seqs[s], **KW)
            try:
                solo.step()
                alone = solo.dense_map(**MAP_KW).extract()
            finally:
                solo.close()
            part = vm.extract(map_id=s)
            assert len(part) > 1000 and (alone["map"] == 0).all() and (part["map"] == s).all()
            _same(part, alone, fields=("ix", "iy", "iz", "count", "x", "y", "z", "intensity"))
    finally:
        vm.close()


def test_dense_map_refuses_what_it_cannot_serve(pipe):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(2, anms_num=500, unique_frames=2, seed=5, with_ba=False)   # depth="match": no disparity maps
    try:
        with pytest.raises(AssertionError):
            p.dense_map()
    finally:
        p.close()


def test_write_ply_round_trip(pipe, tmp_path):
    from stereo_visual_slam_amd.dense import read_ply, write_ply
    vm = pipe.dense_map(step=4, **MAP_KW)
    try:
        v = vm.extract()
    finally:
        vm.close()
    path = str(tmp_path / "map.ply")
    write_ply(path, v)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)) and len(raw) == raw.index(b"end_header\n") + 11 + 20 * len(v)
    back = read_ply(path)
    assert len(back) == len(v) > 100
    for f in ("x", "y", "z", "intensity", "count"):
        assert np.array_equal(back[f].view(np.uint32), v[f].view(np.uint32)), f
