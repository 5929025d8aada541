"""GPU: KeyframePipeline.surface_remap() -- the last step's frames taken out of the surface map and re-integrated at corrected poses -- against
clear() + surface_map(poses=...) on the blocks of the latter; thresholds that move some frames or none; a second remap back to the first poses; the
refusals.  The configuration of tests/test_gpu_surface_map.py: full-size frames, two segments of three, the side tests' gates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KW = dict(anms_num=500, n_kf=3, unique_frames=3, seed=5, ba_windows="tracks", depth="sgbm")
SEGMENTS = [3, 3]
MAP_KW = dict(voxel_size=0.2, trunc_voxels=4, log2_blocks=15)
LEAN = dict(z_min=10.0, z_max=20.0, step=2)


def _as_dict(blocks):
    ids, vox = blocks
    return {tuple(k): v for k, v in zip(ids.tolist(), vox)}


def _differ_on(got, want):
    """the voxels in which the map `got` differs from `want`, over want's blocks (all of which got must hold)"""
    return sum(int((got[k] != v).any(-1).sum()) for k, v in want.items())


@pytest.fixture(scope="module")
def pipe():
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    p = KeyframePipeline(sum(SEGMENTS), segments=SEGMENTS, **KW)
    p.step()
    yield p
    p.close()


@pytest.fixture(scope="module")
def story(pipe):
    """one map through the whole sequence, every state downloaded once: integrated, remapped to perturbed poses, a remap that moves nothing, a remap of
    the frames beyond a threshold back to the first poses, the rest back; then the map cleared and integrated afresh at the poses each state stands for"""
    from stereo_visual_slam_amd import synth
    p = pipe
    rng = np.random.default_rng(3)
    first = p.trajectories()
    poses = [(ids, np.stack([synth.perturb_pose(t, rng, 0.01) for t in Ts])) for ids, Ts in first]
    out = dict(poses=poses)
    tm = p.surface_map(**MAP_KW, **LEAN)
    try:
        out["T0"], out["ids0"] = (a.copy() for a in (p.surface_frames["T"], p.surface_frames["map_id"]))
        out["reach0"] = p.surface_frames["reach"].cpu().tolist()
        out["orig"], out["n_orig"] = _as_dict(tm.blocks()), tm.stats()["n_blocks"]
        out["moved"] = p.surface_remap(poses)
        out["remapped"], out["status"] = _as_dict(tm.blocks()), tm.stats()["status"]
        out["T1"], out["reach1"] = p.surface_frames["T"].copy(), p.surface_frames["reach"].cpu().tolist()
        out["n_remapped"] = tm.stats()["n_blocks"]
        out["none"] = p.surface_remap(first, min_shift=1e3, min_turn=4.0)
        out["after_none"] = _as_dict(tm.blocks())
        # the camera centres' shifts back to the first poses, and a threshold between them
        C = lambda T: -np.einsum("bji,bj->bi", np.stack([synth.R_from_quat(q) for q in T[:, :4]]), T[:, 4:])
        shift = np.linalg.norm(C(out["T1"]) - C(out["T0"]), axis=1)
        out["shift"], out["cut"] = shift, float(np.sort(shift)[2:4].mean())
        out["some"] = p.surface_remap(first, min_shift=out["cut"], min_turn=4.0)
        out["partial"], out["T_partial"] = _as_dict(tm.blocks()), p.surface_frames["T"].copy()
        out["rest"] = p.surface_remap(first)
        out["back"], out["status_back"] = _as_dict(tm.blocks()), tm.stats()["status"]
        out["T_back"] = p.surface_frames["T"].copy()
        # the yardsticks: the same map cleared and integrated afresh
        as_poses = lambda T: [(ids, T[f0 + ids]) for (ids, _), f0 in zip(first, np.cumsum([0] + SEGMENTS[:-1]))]
        for name, T in (("fresh_new", out["T1"]), ("fresh_partial", out["T_partial"])):
            tm.clear()
            assert p.surface_map(tsdf_map=tm, poses=as_poses(T), **LEAN) is tm
            out[name] = _as_dict(tm.blocks())
    finally:
        tm.close()
    return out


def test_surface_map_remembers_what_it_integrated(pipe, story):
    T, map_id = pipe.dense_map_inputs()
    assert np.array_equal(story["T0"], T) and np.array_equal(story["ids0"], map_id) and map_id.tolist() == [0, 0, 0, 1, 1, 1]
    assert story["reach0"] == [story["n_orig"]] * 6 and story["n_orig"] == len(story["orig"]) > 200


def test_remap_equals_a_fresh_map_at_the_new_poses(pipe, story):
    tm_n = story["moved"]
    assert tm_n[1] == 6 and story["status"] == 0
    T_want, _ = pipe.dense_map_inputs(story["poses"])
    assert np.array_equal(story["T1"], T_want) and story["reach1"] == [story["n_remapped"]] * 6 and story["n_remapped"] >= story["n_orig"]
    fresh = story["fresh_new"]
    assert len(fresh) > 200 and set(fresh) <= set(story["remapped"])
    assert _differ_on(story["remapped"], fresh) == 0
    assert _differ_on(story["remapped"], story["orig"]) > 1000, "the move must matter"


def test_a_threshold_above_every_motion_moves_nothing(story):
    assert story["none"][1] == 0
    assert story["after_none"].keys() == story["remapped"].keys() and _differ_on(story["after_none"], story["remapped"]) == 0


def test_a_threshold_between_the_motions_moves_the_frames_beyond_it(story):
    n = int((story["shift"] > story["cut"]).sum())
    assert 0 < n < 6 and story["some"][1] == n
    moved = story["shift"] > story["cut"]
    assert np.array_equal(story["T_partial"], np.where(moved[:, None], story["T0"], story["T1"]))
    assert _differ_on(story["partial"], story["fresh_partial"]) == 0


def test_remapping_back_restores_the_first_sums(story):
    assert story["rest"][1] == 6 - story["some"][1] and story["status_back"] == 0
    assert np.array_equal(story["T_back"], story["T0"])
    assert _differ_on(story["back"], story["orig"]) == 0


def test_surface_remap_refuses_what_it_cannot_serve(pipe, story, monkeypatch):
    other = pipe.vo.tsdf_map(0.2, 4, 6)
    try:
        with pytest.raises(AssertionError):
            pipe.surface_remap(story["poses"], tsdf_map=other)          # not the map the last surface_map() filled
    finally:
        other.close()
    with pytest.raises(AssertionError):
        pipe.surface_remap(story["poses"])                              # that map is closed
    monkeypatch.delattr(pipe, "surface_frames")
    with pytest.raises(AssertionError):
        pipe.surface_remap(story["poses"])                              # no surface_map() before it
