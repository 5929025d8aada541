"""The keyframe gate inside the map-based pose passes (keyframe_gate="per_pass"), without a GPU: the CPU restatement of tests/gated_map_ref.py on a
hand-worked table (a non-keyframe creates nothing, the tracked inlier count decays below 80 and makes a keyframe), the pass semantics against the
sequential loop on random tables (F - 1 passes reproduce it exactly, states flip between passes), the all-keyframe case against
tests/pose_map_ref.py, and the pipeline's refusals."""
import numpy as np
import pytest

import gated_map_ref as GR
import kf_gate_ref as KR
import pose_map_ref as PR
from test_gpu_windows import _random_tracks


def dense_tracks(rng, F, cap):
    """_random_tracks with every keypoint slot used, a depth association for each, most depths valid and 75-100 % of the keypoints matched into the
    next frame: enough inputs per frame pair for the gate's 80 inliers to matter"""
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = _random_tracks(rng, F, cap, cap)
    nk[:] = cap
    kps["x"] = rng.uniform(0, 1241, (F, cap)).astype(np.float32); kps["y"] = rng.uniform(0, 376, (F, cap)).astype(np.float32)
    for f in range(F):
        lr["queryIdx"][f] = rng.permutation(cap); nlr[f] = cap
    valid = (rng.random((F, cap)) < rng.uniform(0.6, 0.95)).astype(np.uint8)
    for i in range(F - 1):
        n = int(cap * rng.uniform(0.75, 1.0))
        f2f["queryIdx"][i, :n] = np.sort(rng.permutation(cap)[:n]); f2f["trainIdx"][i, :n] = rng.permutation(cap)[:n]; nf2f[i] = n
    return kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk


def _tz(z):
    return np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, z])


def hand_table():
    """5 frames, 128 keypoint slots, frame-to-frame matches slot s -> slot s.  Frame 0: slots 0..99 a depth (slot 0 unreliable: landmark A, the others
    reliable).  Frame 1: slot 0 a reliable depth of its own (A tracked), slot 100 a depth (no track reaches it).  Frame 2: no depth.  Frame 3: slot 0
    a reliable depth, slot 101 a depth.  Frame 4: no depth.  Items 0 and 2 match slots 0..99, item 1 slots 0..100, item 3 slots 0..101.
    Pose-stage tables (pass 0): every own-depth input an inlier, T_rel = 0.1 m along z."""
    import oracle as O
    F, cap = 5, 128
    kps = np.zeros((F, cap), O.KEYPOINT_DTYPE)
    kps["x"] = 20.0 + 9.0 * np.arange(cap)[None, :] + 0.5 * np.arange(F)[:, None]
    kps["y"] = 50.0 + 2.0 * (np.arange(cap)[None, :] % 100) + 1.0 * np.arange(F)[:, None]
    lr = np.zeros((F, cap), O.DMATCH_DTYPE); nlr = np.full(F, cap, np.int32)
    lr["queryIdx"] = np.arange(cap)[None, :]; lr["trainIdx"] = np.arange(cap)[None, :]
    xyz = np.zeros((F, cap, 3), np.float32); valid = np.zeros((F, cap), np.uint8); rel = np.zeros((F, cap), np.uint8)
    s = np.arange(100)
    xyz[0, :100] = np.stack([0.1 * s - 5.0, 0.02 * s - 1.0, 10.0 + 0.1 * s], 1); valid[0, :100] = 1; rel[0, 1:100] = 1
    xyz[1, 0] = (-5.0, -1.0, 9.5); valid[1, 0] = 1; rel[1, 0] = 1
    xyz[1, 100] = (2.0, 0.5, 12.0); valid[1, 100] = 1; rel[1, 100] = 1
    xyz[3, 0] = (-5.0, -1.0, 9.8); valid[3, 0] = 1; rel[3, 0] = 1
    xyz[3, 101] = (3.0, 0.5, 14.0); valid[3, 101] = 1; rel[3, 101] = 1
    f2f = np.zeros((F - 1, cap), O.DMATCH_DTYPE); nf2f = np.array([100, 101, 100, 102], np.int32)
    f2f["queryIdx"] = np.arange(cap)[None, :]; f2f["trainIdx"] = np.arange(cap)[None, :]
    inl = np.ones((F - 1, cap), np.uint8)
    T_rel = np.stack([_tz(-0.1)] * (F - 1))
    return kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, np.full(F, cap, np.int32)


HAND_INLIERS = (100, 85, 75, 1000)   # per item: the first n inputs are inliers


def _hand_solver(i, xyz, uv, guess):
    """frame f = i + 1 sits 0.1 m further along z per frame (no rotation: angleY 0); the first HAND_INLIERS[i] inputs are inliers"""
    return _tz(-0.1 * (i + 1)), np.arange(len(uv)) < HAND_INLIERS[i]


def test_hand_worked_table():
    t = hand_table()
    s = GR.sequential(t, _hand_solver, n_kf=4)
    assert np.allclose(s["G"][:, 6], [0, -0.1, -0.2, -0.3, -0.4])
    it = s["items"]
    # 100 tracked inliers into frame 1 (>= 80, angleY 0): frame 1 is no keyframe; 85 into frame 2: none either; 75 into frame 3: below 80, a keyframe
    assert [x["n"] for x in it] == [100, 100, 85, 76]
    assert [int(x["mask"].sum()) for x in it] == [100, 85, 75, 76]
    assert s["state"].tolist() == [2, 1, 1, 2, 2]
    # frame 1 is no keyframe: its own-depth keypoint in slot 100 created no landmark, so frame 2's match of it is no pose input
    assert it[1]["index"][100] == -1 and it[1]["index"][:100].tolist() == list(range(100))
    # frame 3 is a keyframe: the landmark it created in slot 101 is an input of frame 4
    assert it[3]["index"][101] == 75 and np.allclose(it[3]["xyz"][75], KR._world(s["G"][3], t[3][3, 101]))
    # A kept its creation point through frame 1 (no reliable upgrade at a non-keyframe) and took frame 3's reliable depth
    assert np.array_equal(it[1]["xyz"][0], t[3][0, 0]) and np.array_equal(it[2]["xyz"][0], t[3][0, 0])
    assert np.allclose(it[3]["xyz"][0], KR._world(s["G"][3], t[3][3, 0]))
    # windows: empty at frames 1 and 2; window 3 holds keyframes {0, 3}: the 100 landmarks of frame 0 (75 seen again at 3) and the one created at 3
    assert s["windows"][1] == {} and s["windows"][2] == {} and s["n_kf"].tolist() == [1, 0, 0, 2, 3]
    assert s["kf_frame"][2].tolist() == [0, -1, -1, -1] and s["kf_frame"][4].tolist() == [0, 3, 4, -1]
    w3 = s["windows"][3]
    assert sorted(len(k) for k in w3) == [1] * 26 + [2] * 75
    a = [v for k, v in w3.items() if k[0][1] == float(t[0]["x"][0, 0])][0]
    assert a[1] == 1 and np.allclose(a[0], KR._world(s["G"][3], t[3][3, 0]))
    assert s["status"] == 0
    # stage A's gate counts own-depth inliers (100, 2, 0, 2: frames 2..4 rejected); the passes replace those states, and F - 1 passes are the loop
    ninl0 = np.array([100, 2, 0, 2])
    assert GR.states0(t, ninl0).tolist() == [2, 1, 0, 0, 0]
    for K in (1, 2, 3, 4):
        p = GR.passes(t, _hand_solver, K, ninl0, n_kf=4)
        assert np.array_equal(p["state"][:K + 1], s["state"][:K + 1]) and np.array_equal(p["G"][:K + 1], s["G"][:K + 1]), K
        for k in range(K):
            a_, b_ = p["per_pass"][-1]["items"][k], s["items"][k]
            assert np.array_equal(a_["index"], b_["index"]) and np.array_equal(a_["xyz"], b_["xyz"]) and np.array_equal(a_["mask"], b_["mask"]), (K, k)
        assert KR.same_windows(p["windows"][:K + 1], s["windows"][:K + 1], rtol=0, atol=0), K
    assert p["status"] == s["status"] and np.array_equal(p["kf_frame"], s["kf_frame"]) and np.array_equal(p["n_kf"], s["n_kf"])


def _with_rejection(solver, item):
    """the solver with at most 5 inliers at one item: that frame fails check_motion_estimation (state 0, status bit 2)"""
    def f(i, xyz, uv, guess):
        T, m = solver(i, xyz, uv, guess)
        if i == item:
            m = np.asarray(m, bool) & (np.cumsum(m) <= 5)
        return T, m
    return f


@pytest.mark.parametrize("seed", range(4))
def test_passes_reproduce_the_sequential_loop(seed):
    """dense random tables, the gate stand-in solver (a pure function of uv and input order): after k passes the poses, states, inputs and masks of
    frames 0..k and windows 0..k are the sequential loop's, and F - 1 passes reproduce it exactly; states flip between passes"""
    rng = np.random.default_rng(800 + seed)
    flips, states = 0, set()
    for case in range(3):
        F = int(rng.integers(6, 13)); cap = int(rng.choice([128, 256])); n_kf = int(rng.integers(2, 11)); policy = case % 2
        t = dense_tracks(rng, F, cap)
        ninl0 = rng.integers(0, 200, F - 1)
        solver = _with_rejection(GR.gate_solver, int(rng.integers(1, F - 1))) if case == 2 else GR.gate_solver
        s = GR.sequential(t, solver, n_kf=n_kf, policy=policy)
        states |= set(s["state"].tolist())
        if case == 2:
            assert 0 in s["state"] and s["status"] & 4
        tag = (seed, case, F, cap, n_kf)
        for K in sorted({1, 2, F - 1}):
            p = GR.passes(t, solver, K, ninl0, n_kf=n_kf, policy=policy)
            assert np.array_equal(p["G"][:K + 1], s["G"][:K + 1]) and np.array_equal(p["state"][:K + 1], s["state"][:K + 1]), (tag, K)
            for i in range(K):
                a, b = p["per_pass"][-1]["items"][i], s["items"][i]
                assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["mask"], b["mask"]), (tag, K, i)
            assert KR.same_windows(p["windows"][:K + 1], s["windows"][:K + 1], rtol=0, atol=0), (tag, K)
            if K == F - 1:
                assert np.array_equal(p["G"], s["G"]) and np.array_equal(p["state"], s["state"]), tag
                assert np.array_equal(p["kf_frame"], s["kf_frame"]) and np.array_equal(p["evicted"], s["evicted"]), tag
                assert np.array_equal(p["n_kf"], s["n_kf"]) and p["status"] == s["status"], tag
                assert KR.same_windows(p["windows"], s["windows"], rtol=0, atol=0), tag
                seq_states = [p["state0"]] + [pp["state"] for pp in p["per_pass"]]
                flips += sum(int((a != b).sum()) for a, b in zip(seq_states, seq_states[1:]))
    assert {1, 2} <= states and flips > 0, (states, flips)


def _all_keyframes(i, xyz, uv, guess):
    """pose_map_ref's stand-in with at most 60 inliers: every frame passes the motion check with 10 to 79 inliers, so every frame is a keyframe"""
    T, m = PR.standin_solver(i, xyz, uv, guess)
    return T, np.asarray(m, bool) & (np.cumsum(m) <= 60)


@pytest.mark.parametrize("seed", range(3))
def test_all_keyframes_is_pose_map_ref(seed):
    """with every state 2 (10..79 inliers everywhere, stage A's counts too) the gated restatement is pose_map_ref's, exactly"""
    rng = np.random.default_rng(900 + seed)
    for case in range(3):
        F = int(rng.integers(4, 12)); cap = 128; n_kf = int(rng.integers(1, 11)); policy = case % 2
        t = dense_tracks(rng, F, cap)
        ninl0 = rng.integers(10, 80, F - 1)
        g, r = GR.sequential(t, _all_keyframes, n_kf=n_kf, policy=policy), PR.sequential(t, _all_keyframes, n_kf=n_kf, policy=policy)
        assert (g["state"] == 2).all(), g["state"]
        assert all(10 <= it["mask"].sum() <= 79 for it in g["items"])
        for K in (1, 2):
            gp, rp = GR.passes(t, _all_keyframes, K, ninl0, n_kf=n_kf, policy=policy), PR.passes(t, _all_keyframes, K, n_kf=n_kf, policy=policy)
            assert (gp["state0"] == 2).all() and (gp["state"] == 2).all()
            for a, b in ((g, r), (gp, rp)):
                assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["kf_frame"], b["kf_frame"]) and np.array_equal(a["evicted"], b["evicted"])
                assert np.array_equal(a["n_kf"], b["n_kf"]) and a["status"] == b["status"]
                assert KR.same_windows(a["windows"], b["windows"], rtol=0, atol=0)
                for x, y in zip(a["items"], b["items"]):
                    assert np.array_equal(x["index"], y["index"]) and np.array_equal(x["xyz"], y["xyz"]) and np.array_equal(x["mask"], y["mask"])
            for x, y in zip(gp["per_pass"][-1]["items"], rp["per_pass"][-1]["items"]):
                assert np.array_equal(x["index"], y["index"]) and np.array_equal(x["xyz"], y["xyz"]) and np.array_equal(x["mask"], y["mask"])


@pytest.mark.parametrize("kw", [dict(pose_inputs="own_depth"), dict(frame_range=(0, 4, 8)), dict(ba_windows="synthetic"), dict(keyframe_gate="per-pass"),
                                dict(keyframe_gate=True), dict(pose_passes=0)])
def test_pipeline_refuses_unsupported_per_pass_options(kw):
    """keyframe_gate="per_pass" needs pose_inputs="map", the device-built windows and no sequence mode; keyframe_gate=True stays refused with the map
    inputs; unknown values are refused -- all before any device work"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    args = dict(ba_windows="tracks", pose_inputs="map", pose_passes=1, keyframe_gate="per_pass")
    args.update(kw)
    with pytest.raises(AssertionError):
        KeyframePipeline(4, **args)
