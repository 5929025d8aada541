"""GPU: KeyframePipeline.surface_map() -- the SGBM disparities and left images of a step integrated into a TSDF at the poses of
dense_map_inputs() -- against the numpy restatement tests/tsdf_ref.py fed with the downloaded disparities, images and poses; per segment against the
pipeline of that segment alone; poses=, tsdf_map=, a frame outside the trajectories, the PLY file, the refusals.  The configuration of
tests/test_gpu_dense_map.py: full-size frames, two segments of three."""
import numpy as np
import pytest

import tsdf_ref as TR

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=3, unique_frames=3, seed=5, ba_windows="tracks", depth="sgbm")   # the smallest depth="sgbm" window configuration of the suite
SEGMENTS = [3, 3]
MAP_KW = dict(voxel_size=0.2, trunc_voxels=4, log2_blocks=15)
LEAN = dict(z_min=10.0, z_max=20.0, step=2)      # the side tests' gates: a fifth of the blocks, the same code


def _same(got, want, fields=None):
    assert len(got) == len(want), (len(got), len(want))
    for f in fields or want.dtype.names:
        bad = np.flatnonzero(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert len(bad) == 0, (f, len(bad), got[bad[:3]], want[bad[:3]])


def _same_blocks(got, want):
    (gi, gv), (wi, wv) = got, want
    assert gi.shape == wi.shape and np.array_equal(gi, wi), (gi.shape, wi.shape)
    assert np.array_equal(gv, wv), int((gv != wv).sum())


@pytest.fixture(scope="module")
def pipe():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(sum(SEGMENTS), segments=SEGMENTS, **KW)
    p.step()
    yield p
    p.close()


@pytest.fixture(scope="module")
def inputs(pipe):
    """the step's disparities and left images on the host, downloaded once"""
    pipe.vo.sync()
    return pipe.d_disp.cpu().numpy(), np.ascontiguousarray(pipe.h_imgs[:pipe.B])


def _restatement(p, inputs, T, map_id, z_min, z_max, step=1, ref=None):
    disp, gray = inputs
    ref = TR.TsdfRef(MAP_KW["voxel_size"], MAP_KW["trunc_voxels"], list(p.vo.params.cam)) if ref is None else ref
    ref.integrate(disp, gray, T, map_id, z_min, z_max, step)
    return ref


def test_surface_map_equals_the_restatement(pipe, inputs):
    p = pipe
    T, map_id = p.dense_map_inputs()
    assert map_id.tolist() == [0, 0, 0, 1, 1, 1], "every frame of both segments is in a trajectory"
    z_min, z_max = p.vo.params.depth_min, p.vo.params.depth_reliable
    ref = _restatement(p, inputs, T, map_id, z_min, z_max)
    want = ref.extract()
    assert len(ref.blocks) > 1000 and len(want) > 5000 and set(want["map"]) == {0, 1}, "a real map: thousands of blocks and surfels, both segments"
    tm = p.surface_map(**MAP_KW)
    try:
        _same_blocks(tm.blocks(), ref.dump())
        _same(tm.extract(), want)
        _same(tm.extract(min_weight=2), ref.extract(min_weight=2))
        st = tm.stats()
        assert (st["n_blocks"], st["n_samples"], st["n_dropped_range"], st["n_dropped_full"], st["n_frames_skipped"], st["status"]) == \
            (len(ref.blocks), ref.n_samples, ref.n_dropped_range, 0, 0, 0), st
    finally:
        tm.close()


def test_tsdf_map_accumulates_and_poses_are_honoured(pipe, inputs):
    """a second step into the same map (here: the same frames at other poses, as close_loops() or full_ba() would return them) equals the
    restatement fed the same two calls"""
    from stereo_visual_slam_amd import synth
    p = pipe
    T, map_id = p.dense_map_inputs()
    rng = np.random.default_rng(3)
    poses = [(ids, np.stack([synth.perturb_pose(t, rng, 0.01) for t in Ts])) for ids, Ts in p.trajectories()]
    T2, map_id2 = p.dense_map_inputs(poses)
    assert np.array_equal(map_id2, map_id) and not np.array_equal(T2, T)
    ref = _restatement(p, inputs, T, map_id, **LEAN)
    once = ref.dump()
    _restatement(p, inputs, T2, map_id, ref=ref, **LEAN)
    tm = p.surface_map(**MAP_KW, **LEAN)
    try:
        _same_blocks(tm.blocks(), once)
        assert p.surface_map(tsdf_map=tm, poses=poses, **LEAN) is tm
        _same_blocks(tm.blocks(), ref.dump())
        _same(tm.extract(), ref.extract())
    finally:
        tm.close()


def test_frames_outside_the_trajectory_contribute_nothing(pipe, inputs, monkeypatch):
    p = pipe
    T, map_id = p.dense_map_inputs()
    map_id[4] = -1                                    # as if frame 4 were in no trajectory (a frame the keyframe gate rejected)
    monkeypatch.setattr(p, "dense_map_inputs", lambda: (T, map_id))
    tm = p.surface_map(**MAP_KW, **LEAN)
    try:
        _same_blocks(tm.blocks(), _restatement(p, inputs, T, map_id, **LEAN).dump())
    finally:
        tm.close()


def test_every_segment_equals_its_pipeline_alone(pipe):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    tm = pipe.surface_map(**MAP_KW, **LEAN)
    try:
        for s, n in enumerate(SEGMENTS):
            solo = KeyframePipeline(n, sequence=pipe.h_seqs[s], **KW)
            try:
                solo.step()
                alone = solo.surface_map(**MAP_KW, **LEAN).extract()
            finally:
                solo.close()
            part = tm.extract(map_id=s)
            assert len(part) > 300 and (alone["map"] == 0).all() and (part["map"] == s).all()
            _same(part, alone, fields=[f for f in part.dtype.names if f != "map"])
    finally:
        tm.close()


def test_surface_map_refuses_what_it_cannot_serve(pipe):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(2, anms_num=500, unique_frames=2, seed=5, with_ba=False)   # depth="match": no disparity maps
    try:
        with pytest.raises(AssertionError):
            p.surface_map()
    finally:
        p.close()
    other = pipe.vo.__class__(device=0, max_batch=1)
    try:
        foreign = other.tsdf_map(0.2, 4, 6)
        with pytest.raises(AssertionError):
            pipe.surface_map(tsdf_map=foreign)
    finally:
        other.close()


def test_write_surfel_ply_round_trip(pipe, tmp_path):
    from stereo_visual_slam_amd.dense import read_surfel_ply, write_surfel_ply
    tm = pipe.surface_map(**MAP_KW, **LEAN)
    try:
        v = tm.extract()
    finally:
        tm.close()
    path = str(tmp_path / "surface.ply")
    write_surfel_ply(path, v)
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)) and len(raw) == raw.index(b"end_header\n") + 11 + 32 * len(v)
    back = read_surfel_ply(path)
    assert len(back) == len(v) > 100
    for f in ("x", "y", "z", "nx", "ny", "nz", "intensity", "weight"):
        assert np.array_equal(back[f].view(np.uint32), v[f].view(np.uint32)), f
    n = np.stack([back["nx"], back["ny"], back["nz"]], 1).astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6
