"""Pose inputs against the map (pose_inputs="map"), without a GPU: the CPU restatement of tests/pose_map_ref.py on a hand-worked table, the pass
semantics against the sequential loop on random tables (F - 1 passes reproduce it exactly), and pass 0 against the pinned oracle's windows."""
import numpy as np
import pytest

import kf_gate_ref as KR
import pose_map_ref as R
from test_gpu_windows import _random_tracks
from test_kf_gate import _sliding_windows


def _tz(z):
    return np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, z])


def hand_table():
    """4 frames, 4 keypoint slots, every frame-to-frame match slot s -> slot s.  Frame 0: slot 0 a depth (unreliable: landmark A), slot 1 a reliable
    depth (B), slot 2 a reliable depth (C).  Frame 1: slot 0 no depth, slot 1 a depth of its own (another triangulation of B), slot 2 no depth.
    Frame 2: slot 0 a reliable depth (A takes it), slot 1 no depth.  Frame 3: nothing.  Items 0, 1, 2 match slots 0 and 1; item 0 also slot 2."""
    import oracle as O
    F, cap = 4, 4
    kps = np.zeros((F, cap), O.KEYPOINT_DTYPE)
    kps["x"] = 100.0 + 50.0 * np.arange(cap)[None, :] + 3.0 * np.arange(F)[:, None]
    kps["y"] = 50.0 + 20.0 * np.arange(cap)[None, :] + 2.0 * np.arange(F)[:, None]
    lr = np.zeros((F, cap), O.DMATCH_DTYPE); nlr = np.full(F, cap, np.int32)
    lr["queryIdx"] = np.arange(cap)[None, :]; lr["trainIdx"] = np.arange(cap)[None, :]
    xyz = np.zeros((F, cap, 3), np.float32); valid = np.zeros((F, cap), np.uint8); rel = np.zeros((F, cap), np.uint8)
    xyz[0, 0] = (1, 0, 10); valid[0, 0] = 1
    xyz[0, 1] = (-1, 0, 20); valid[0, 1] = 1; rel[0, 1] = 1
    xyz[0, 2] = (0, 1, 15); valid[0, 2] = 1; rel[0, 2] = 1
    xyz[1, 1] = (-1, 0, 18.5); valid[1, 1] = 1; rel[1, 1] = 1
    xyz[2, 0] = (1, 0, 8.2); valid[2, 0] = 1; rel[2, 0] = 1
    f2f = np.zeros((F - 1, cap), O.DMATCH_DTYPE); nf2f = np.array([3, 2, 2], np.int32)
    f2f["queryIdx"] = np.arange(cap)[None, :]; f2f["trainIdx"] = np.arange(cap)[None, :]
    inl = np.ones((F - 1, cap), np.uint8)
    T_rel = np.stack([_tz(-1.0)] * (F - 1))
    return kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, np.full(F, cap, np.int32)


def _hand_solver(i, xyz, uv, guess):
    """every input an inlier; frame f = i + 1 sits 1 m further along z per frame"""
    return _tz(-(i + 1.0)), np.ones(len(uv), bool)


def test_hand_worked_table():
    t = hand_table()
    s = R.sequential(t, _hand_solver, n_kf=4)
    assert np.allclose(s["G"][:, 6], [0, -1, -2, -3])
    it = s["items"]
    # item 0: slots 0, 1, 2 of frame 0 are features (created there): three inputs at their creation points, uv = the frame-1 keypoints
    assert it[0]["index"][:3].tolist() == [0, 1, 2] and it[0]["n"] == 3
    assert np.array_equal(it[0]["xyz"], np.array([[1, 0, 10], [-1, 0, 20], [0, 1, 15]], np.float32))
    assert np.array_equal(it[0]["uv"], np.stack([t[0]["x"][1, :3], t[0]["y"][1, :3]], 1))
    # item 1: slot 0 of frame 1 has no depth of its own -- an input at its landmark's position; slot 1 has one (18.5 m: 19.5 m in the world) and is still
    # located at its landmark's position (20 m), not at its own triangulation; slot 2 of frame 1 (tracked, no depth) is not matched on
    assert it[1]["n"] == 2 and it[1]["index"][:2].tolist() == [0, 1]
    assert np.array_equal(it[1]["xyz"], np.array([[1, 0, 10], [-1, 0, 20]], np.float32))
    # item 2: A took frame 2's reliable depth (8.2 m at 2 m: 10.2 m in the world); B keeps its first reliable position
    assert np.allclose(it[2]["xyz"], [[1, 0, 10.2], [-1, 0, 20]], atol=1e-5) and it[2]["n"] == 2
    # the windows: A and B seen in every frame, C in frames 0 and 1, A reliable from frame 2 on
    w = s["windows"][3]
    obs = {len(k): v for k, v in w.items()}
    assert sorted(len(k) for k in w) == [2, 4, 4]
    assert obs[2][1] == 1 and np.allclose(obs[2][0], [0, 1, 15])
    # the passes: pass 0 is the own-depth stage (the chain of T_rel is the same motion), and F - 1 passes are the sequential loop
    for K in (1, 2, 3):
        p = R.passes(t, _hand_solver, K, n_kf=4)
        assert np.array_equal(p["G"], s["G"])
        assert KR.same_windows(p["windows"], s["windows"], rtol=0, atol=0)
        for a, b in zip(p["per_pass"][-1]["items"], s["items"]):
            assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["uv"], b["uv"])


def test_hand_worked_table_stops_a_track_at_an_outlier():
    """an outlier of the map problem erases the feature (:306): the link out of it continues nothing, and a frame with no inlier keeps the last pose"""
    t = hand_table()

    def solver(i, xyz, uv, guess):
        m = np.ones(len(uv), bool)
        if i == 0:
            m[0] = False            # A's match into frame 1 is an outlier
        if i == 2:
            m[:] = False            # frame 3: no model
        return _tz(-(i + 1.0)), m
    s = R.sequential(t, solver, n_kf=4)
    assert s["items"][1]["n"] == 1 and s["items"][1]["index"][:2].tolist() == [-1, 0]   # slot 0 of frame 1 is no feature
    assert np.array_equal(s["G"][3], s["G"][2])
    assert np.array_equal(R.passes(t, solver, 3, n_kf=4)["G"], s["G"])


def _count_links(items):
    return sum(int(it["mask"].sum()) for it in items)


@pytest.mark.parametrize("seed", range(4))
def test_passes_reproduce_the_sequential_loop(oracle, seed):
    """random tables, the stand-in solver (a pure function of uv and input order): after k passes frames 0..k are the sequential loop's, and F - 1
    passes reproduce it -- poses, every pass's inputs and masks, and the windows -- exactly"""
    rng = np.random.default_rng(700 + seed)
    n_links = 0
    for case in range(6):
        F = int(rng.integers(4, 14)); cap = int(rng.choice([32, 64])); n_kf = int(rng.integers(1, 11)); policy = int(case % 2)
        t = _random_tracks(rng, F, cap, cap)
        s = R.sequential(t, R.standin_solver, n_kf=n_kf, policy=policy)
        n_links += _count_links(s["items"])
        tag = (seed, case, F, cap, n_kf)
        for K in sorted({1, 2, F - 1}):
            p = R.passes(t, R.standin_solver, K, n_kf=n_kf, policy=policy)
            k = min(K, F - 1)
            assert np.array_equal(p["G"][:k + 1], s["G"][:k + 1]), (tag, K)
            for i in range(k):
                a, b = p["per_pass"][-1]["items"][i], s["items"][i]
                assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["mask"], b["mask"]), (tag, K, i)
            if K == F - 1:
                assert np.array_equal(p["G"], s["G"]), tag
                assert np.array_equal(p["kf_frame"], s["kf_frame"]) and np.array_equal(p["evicted"], s["evicted"]), tag
                assert KR.same_windows(p["windows"], s["windows"], rtol=0, atol=0), tag
    assert n_links > 30, n_links


@pytest.mark.parametrize("seed", range(3))
def test_pass0_windows_match_oracle(oracle, seed):
    """no refinement pass: the windows on (G^0, links^0) are oracle.build_windows' (the sliding window, every frame a keyframe), under both track rules"""
    rng = np.random.default_rng(900 + seed)
    for case in range(4):
        F = int(rng.integers(1, 20)); cap = int(rng.choice([32, 64])); n_kf = int(rng.integers(1, 12)); thr = (4.0, 300.0)[case % 2]
        rule = 1 if case < 3 else 0
        t = _random_tracks(rng, F, cap, int(rng.integers(1, cap + 1)))
        p = R.passes(t, R.standin_solver, 0, n_kf=n_kf, reproj_thr=thr, track_rule=rule)
        out = oracle.build_windows(*t[:10], n_kf=n_kf, lm_capacity=F * cap * (n_kf + 1), edge_capacity=2 * F * cap * (n_kf + 1), reproj_thr=thr,
                                   track_rule=rule)
        assert out["status"] == 0
        assert KR.same_windows(p["windows"], _sliding_windows(out, F, n_kf)), (seed, case, F, cap, n_kf)


@pytest.mark.parametrize("kw", [dict(ba_windows="synthetic"), dict(keyframe_gate=True), dict(frame_range=(0, 4, 8)), dict(pose_passes=0),
                                dict(pose_inputs="frame")])
def test_pipeline_refuses_unsupported_map_options(kw):
    """pose_inputs="map" needs the device-built windows and at least one pass; the keyframe gate and sequence mode are out of scope (refused before any
    device work)"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    args = dict(ba_windows="tracks", pose_inputs="map", pose_passes=1)
    args.update(kw)
    with pytest.raises(AssertionError):
        KeyframePipeline(4, **args)
