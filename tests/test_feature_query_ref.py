"""The reference's frame-to-frame query set inside the gated map passes (f2f_queries="features"), without a GPU: the CPU restatement of
tests/feature_query_ref.py -- the pass semantics against the sequential loop on random tables whose pair tables are matched inside the loop by the
oracle's matcher (after k passes frames 0..k and tables 0..k-1 are the loop's, F - 1 passes reproduce it), the all-features case against
tests/gated_map_ref.py -- and the public surface: the header declares the two new entries, SIGNATURES lists them, the pipeline refuses the option
outside pose_inputs="map" + keyframe_gate="per_pass"."""
import os
import re

import numpy as np
import pytest

import feature_query_ref as FQ
import gated_map_ref as GR
import kf_gate_ref as KR
from test_gated_map_ref import _all_keyframes, dense_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vslam_feature_matching_subset_dev", "vslam_build_map_pnp_inputs_requery_dev")


def planted_descriptors(rng, F, cap, keep=0.8, flips=6):
    """random 256-bit descriptors; a `keep` share of frame f's rows reappear in frame f + 1 at shuffled slots with up to `flips` bits flipped (true
    correspondences at small distances), and a tenth of every frame's rows are near-duplicates of another row of the SAME frame (two or three bits
    apart), so that which of them is a query decides who wins the cross-check"""
    desc = np.zeros((F, cap, 32), np.uint8)
    desc[0] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    for f in range(F):
        if f > 0:
            desc[f] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
            src = rng.permutation(cap)[:int(keep * cap)]; dst = rng.permutation(cap)[:len(src)]
            desc[f, dst] = desc[f - 1, src]
            for d in dst:
                for b in rng.integers(0, 256, int(rng.integers(0, flips + 1))):
                    desc[f, d, b // 8] ^= np.uint8(1 << (b % 8))
        dup = rng.permutation(cap)[:cap // 5]
        a, b_ = dup[:len(dup) // 2], dup[len(dup) // 2:2 * (len(dup) // 2)]
        desc[f, b_] = desc[f, a]
        for d in b_:
            for b in rng.integers(0, 256, int(rng.integers(2, 4))):
                desc[f, d, b // 8] ^= np.uint8(1 << (b % 8))
    return desc


def matched_tracks(rng, O, F, cap, valid_share=None):
    """dense_tracks whose pose-stage table is the oracle's all-keypoint match of planted descriptors"""
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = dense_tracks(rng, F, cap)
    if valid_share is not None:
        valid = (rng.random((F, cap)) < valid_share).astype(np.uint8)
    desc = planted_descriptors(rng, F, cap)
    f2f = np.zeros((F - 1, cap), O.DMATCH_DTYPE); nf2f = np.zeros(F - 1, np.int32)
    for i in range(F - 1):
        m = O.feature_matching(desc[i], desc[i + 1], 1.0)
        f2f[i, :len(m)] = m; nf2f[i] = len(m)
    return (kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk), desc


def _same_item(a, b):
    return np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["uv"], b["uv"]) and np.array_equal(a["mask"], b["mask"])


@pytest.mark.parametrize("seed", range(3))
def test_passes_reproduce_the_sequential_loop(oracle, seed):
    """after K passes the tables of pairs 0..K-1 and the feature lists, inputs, masks, poses, states and windows of frames 0..K are the sequential
    loop's, F - 1 passes reproduce it everywhere; the feature-query tables differ from the all-keypoint ones and both gate states occur"""
    rng = np.random.default_rng(4100 + seed)
    states, differ = set(), 0
    for case in range(2):
        F = int(rng.integers(5, 9)); cap = int(rng.choice([256, 384])); n_kf = int(rng.integers(2, 8)); policy = case % 2
        t, desc = matched_tracks(rng, oracle, F, cap, valid_share=rng.uniform(0.3, 0.9))   # (enough inputs for the gate's 80 inliers to matter)
        match = FQ.oracle_matcher(oracle, desc, t[10])
        ninl0 = rng.integers(0, 200, F - 1)
        s = FQ.sequential(t, match, GR.gate_solver, n_kf=n_kf, policy=policy)
        states |= set(s["state"].tolist())
        for i in range(F - 1):
            all_kp = t[6][i, :t[7][i]]
            differ += int(len(all_kp) != len(s["tables"][i]) or not np.array_equal(all_kp, s["tables"][i]))
            assert set(s["tables"][i]["queryIdx"].tolist()) <= set(s["feats"][i].tolist())
        tag = (seed, case, F, cap)
        for K in range(1, F):
            p = FQ.passes(t, match, GR.gate_solver, K, ninl0, n_kf=n_kf, policy=policy)
            last = p["per_pass"][-1]
            assert np.array_equal(p["G"][:K + 1], s["G"][:K + 1]) and np.array_equal(p["state"][:K + 1], s["state"][:K + 1]), (tag, K)
            for i in range(K):
                assert np.array_equal(last["tables"][i], s["tables"][i]) and np.array_equal(last["feats"][i], s["feats"][i]), (tag, K, i)
                assert _same_item(last["items"][i], s["items"][i]), (tag, K, i)
            assert KR.same_windows(p["windows"][:K + 1], s["windows"][:K + 1], rtol=0, atol=0), (tag, K)
            if K == F - 1:
                assert np.array_equal(p["G"], s["G"]) and np.array_equal(p["state"], s["state"]), tag
                assert np.array_equal(p["kf_frame"], s["kf_frame"]) and np.array_equal(p["evicted"], s["evicted"]), tag
                assert np.array_equal(p["n_kf"], s["n_kf"]) and p["status"] == s["status"], tag
                assert KR.same_windows(p["windows"], s["windows"], rtol=0, atol=0), tag
                for f in range(F):
                    assert np.array_equal(p["feats"][f], s["feats"][f]), (tag, f)
    assert {1, 2} <= states and differ > 0, (states, differ)


@pytest.mark.parametrize("seed", range(2))
def test_all_features_is_gated_map_ref(oracle, seed):
    """every keypoint depth-valid and every state 2 (10..79 inliers everywhere): every keypoint is a feature, every pair's table is the all-keypoint
    one, and the model is gated_map_ref's on those tables, exactly -- with the oracle's matcher inside the loop and with the fixed tables"""
    rng = np.random.default_rng(4200 + seed)
    F = int(rng.integers(4, 8)); cap = 128; n_kf = int(rng.integers(2, 8))
    t, desc = matched_tracks(rng, oracle, F, cap, valid_share=2.0)
    ninl0 = rng.integers(10, 80, F - 1)
    g = GR.sequential(t, _all_keyframes, n_kf=n_kf)
    assert (g["state"] == 2).all()
    for match in (FQ.oracle_matcher(oracle, desc, t[10]), FQ.fixed_tables(t)):
        s = FQ.sequential(t, match, _all_keyframes, n_kf=n_kf)
        assert all(np.array_equal(s["feats"][f], np.arange(cap)) for f in range(F))
        assert all(np.array_equal(s["tables"][i], t[6][i, :t[7][i]]) for i in range(F - 1))
        for K in (1, 2):
            gp, sp = GR.passes(t, _all_keyframes, K, ninl0, n_kf=n_kf), FQ.passes(t, match, _all_keyframes, K, ninl0, n_kf=n_kf)
            for a, b in ((g, s), (gp, sp)):
                assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["state"], b["state"]) and np.array_equal(a["kf_frame"], b["kf_frame"])
                assert np.array_equal(a["n_kf"], b["n_kf"]) and a["status"] == b["status"] and KR.same_windows(a["windows"], b["windows"], rtol=0, atol=0)
            for x, y in zip(g["items"], s["items"]):
                assert _same_item(x, y) and np.array_equal(x["index"][:y["n"]], y["index"])
            for x, y in zip(gp["per_pass"][-1]["items"], sp["per_pass"][-1]["items"]):
                assert _same_item(x, y)


def test_header_and_signature_table_declare_the_new_entries(pkg):
    hdr = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = pkg.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in pkg.SIGNATURES and name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
    assert hasattr(pkg.VO, "feature_matching_subset_dev") and hasattr(pkg.VO, "build_map_pnp_inputs_requery_dev")
    names = lib.vslam_kernel_names().decode().split()
    assert "match_train_nearest_sel_kernel" in names and "track_features_kernel" in names


@pytest.mark.parametrize("kw", [dict(pose_inputs="own_depth", keyframe_gate=False), dict(keyframe_gate=False), dict(keyframe_gate=True, pose_inputs="own_depth"),
                                dict(f2f_queries="feature"), dict(f2f_queries=True)])
def test_pipeline_refuses_feature_queries_outside_per_pass(kw):
    """f2f_queries="features" needs pose_inputs="map" and keyframe_gate="per_pass"; unknown values are refused -- all before any device work"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    args = dict(ba_windows="tracks", pose_inputs="map", pose_passes=1, keyframe_gate="per_pass", f2f_queries="features")
    args.update(kw)
    with pytest.raises(AssertionError):
        KeyframePipeline(4, **args)
