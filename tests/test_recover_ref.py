"""The reference's failure handling inside the gated map passes (rejected_frames="recover"), without a GPU: the CPU restatement of
tests/recover_ref.py -- its reduction to tests/feature_query_ref.py when nothing is rejected, the pass semantics against the sequential loop
(contract (B): after k passes frames 0..k are the loop's, F - 1 passes reproduce it) on planted rejection patterns with two stand-in solvers and
descriptors whose distances make the frame gap matter -- and the public surface: the header declares the new entries, SIGNATURES lists them, the
pipeline refuses the option outside pose_inputs="map" + keyframe_gate="per_pass" + f2f_queries="features"."""
import os
import re

import numpy as np
import pytest

import feature_query_ref as FQ
import gated_map_ref as GR
import kf_gate_ref as KR
import recover_ref as RR
from test_gated_map_ref import _all_keyframes, dense_tracks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("vslam_frame_pairs_dev", "vslam_feature_matching_pairs_dev", "vslam_gate_states_pairs_dev", "vslam_build_map_pnp_inputs_recover_dev",
               "vslam_build_windows_map_recover_dev")

# planted rejection patterns: (F, rejected frames).  A single frame, a run of three and a frame directly after frame 0; a run of exactly ten,
# recovered at gap 11; a run of eleven: Lost (frame 0, an accepted frame, the run, then the Lost frames: F >= 14)
PATTERNS = {"single_and_run": (12, (1, 4, 7, 8, 9)), "run10": (14, tuple(range(2, 12))), "run11": (15, tuple(range(2, 13)))}


def planned_pred(F, rejected):
    """the last accepted frame before f when exactly `rejected` are rejected (Lost frames: the frame before)"""
    pred, last = np.full(F, -1, np.int32), 0
    for f in range(1, F):
        pred[f] = last if f - last <= RR.LOST_RUN + 1 else f - 1
        if f not in rejected:
            last = f
    return pred


def planted_gap_descriptors(rng, F, cap, pred, keep=0.8, far=0.3):
    """test_feature_query_ref.planted_descriptors with frame f's surviving rows copied from frame pred[f] -- the frame it will be matched against --
    and a `far` share of them carrying 31-59 flipped bits (distinct bits): beyond the gate of a gap-1 pair (max(2 d_min, 30) with d_min ~ 0), inside
    that of a pair of gap >= 2 (60 and more).  The others carry up to 6; a tenth of every frame's rows are near-duplicates of another row."""
    desc = np.zeros((F, cap, 32), np.uint8)
    for f in range(F):
        desc[f] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
        if f > 0:
            src = rng.permutation(cap)[:int(keep * cap)]; dst = rng.permutation(cap)[:len(src)]
            desc[f, dst] = desc[pred[f], src]
            for d in dst:
                n = int(rng.integers(31, 60)) if rng.random() < far else int(rng.integers(0, 7))
                for b in rng.permutation(256)[:n]:
                    desc[f, d, b // 8] ^= np.uint8(1 << (b % 8))
        dup = rng.permutation(cap)[:cap // 5]
        a, b_ = dup[:len(dup) // 2], dup[len(dup) // 2:2 * (len(dup) // 2)]
        desc[f, b_] = desc[f, a]
        for d in b_:
            for b in rng.integers(0, 256, int(rng.integers(2, 4))):
                desc[f, d, b // 8] ^= np.uint8(1 << (b % 8))
    return desc


def recover_tracks(rng, O, F, cap, rejected, valid_share=None):
    """dense_tracks whose pose-stage table is the oracle's all-keypoint match of ADJACENT frames at gap 1, on descriptors planted for the pairing that
    rejecting exactly `rejected` gives"""
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = dense_tracks(rng, F, cap)
    if valid_share is not None:
        valid = (rng.random((F, cap)) < valid_share).astype(np.uint8)
    desc = planted_gap_descriptors(rng, F, cap, planned_pred(F, rejected))
    f2f = np.zeros((F - 1, cap), O.DMATCH_DTYPE); nf2f = np.zeros(F - 1, np.int32)
    for i in range(F - 1):
        m = O.feature_matching(desc[i], desc[i + 1], 1.0)
        f2f[i, :len(m)] = m; nf2f[i] = len(m)
    return (kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk), desc


def planted_solver(rejected):
    """(a) gated_map_ref.gate_solver, except that for the frames in `rejected` it keeps only the first five inliers: fewer than the 10 that
    check_motion_estimation asks for.  A pure function of (i, xyz, uv)."""
    def solve(i, xyz, uv, guess):
        T, m = GR.gate_solver(i, xyz, uv, guess)
        if (i + 1) in rejected:
            m = np.asarray(m, bool) & (np.cumsum(m) <= 5)
        return T, m
    return solve


def count_solver(threshold):
    """(b) gate_solver, keeping five inliers whenever the item has fewer than `threshold` inputs: the input count hangs on the feature list of the
    frame matched against, which changes from pass to pass, and so do the states.  A pure function of (i, xyz, uv)."""
    def solve(i, xyz, uv, guess):
        T, m = GR.gate_solver(i, xyz, uv, guess)
        if len(uv) < threshold:
            m = np.asarray(m, bool) & (np.cumsum(m) <= 5)
        return T, m
    return solve


def _same_item(a, b):
    return np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["uv"], b["uv"]) and np.array_equal(a["mask"], b["mask"])


def check_contract_b(p, s, K, F, tag):
    """after K passes everything that belongs to frames 0..K is the sequential loop's"""
    last = p["per_pass"][-1]
    assert np.array_equal(p["G"][:K + 1], s["G"][:K + 1]) and np.array_equal(p["state"][:K + 1], s["state"][:K + 1]), (tag, K)
    assert np.array_equal(last["pred"][:K + 1], s["pred"][:K + 1]) and np.array_equal(last["gap"][:K], s["gap"][:K]), (tag, K)
    for i in range(K):
        assert np.array_equal(last["tables"][i], s["tables"][i]) and np.array_equal(last["feats"][i], s["feats"][i]), (tag, K, i)
        assert _same_item(last["items"][i], s["items"][i]), (tag, K, i)
    assert KR.same_windows(p["windows"][:K + 1], s["windows"][:K + 1], rtol=0, atol=0), (tag, K)
    if K == F - 1:
        for k in ("G", "state", "kf_frame", "evicted", "n_kf", "pred", "gap"):
            assert np.array_equal(p[k], s[k]), (tag, k)
        assert p["status"] == s["status"] and KR.same_windows(p["windows"], s["windows"], rtol=0, atol=0), tag
        for f in range(F):
            assert np.array_equal(p["feats"][f], s["feats"][f]), (tag, f)


def gap_matters(O, desc, nkps, s):
    """pairs of the sequential result with gap >= 2 whose table holds a match with 30 < distance <= 30 gap that the same pair matched at gap 1 lacks"""
    match, n = RR.oracle_matcher(O, desc, nkps), 0
    for f in range(1, len(s["pred"])):
        l, g = int(s["pred"][f]), s["gap"][f - 1]
        if l < 0 or g < 2:
            continue
        tab = s["tables"][f - 1]
        wide = tab[(tab["distance"] > 30) & (tab["distance"] <= 30 * g)]
        narrow = match(l, f, s["feats"][l], 1.0)
        have = set(zip(narrow["queryIdx"].tolist(), narrow["trainIdx"].tolist()))
        n += int(any((q, t) not in have for q, t in zip(wide["queryIdx"].tolist(), wide["trainIdx"].tolist())))
    return n


@pytest.mark.parametrize("seed", range(2))
def test_nothing_rejected_is_feature_query_ref(oracle, seed):
    """solvers that never reject on stage-A counts that reject nothing (10..79 inliers: every frame a keyframe, so every frame has features and every
    item inputs): sequential and passes equal feature_query_ref's, exactly, with pred = f - 1.  A pass of feature_query_ref's in which a frame comes
    out rejected all the same (too few inputs in an early pass) is where the two models part, and is left out."""
    rng = np.random.default_rng(7100 + seed)
    F = int(rng.integers(5, 9)); cap = 128; n_kf = int(rng.integers(2, 8)); policy = seed % 2
    t, desc = recover_tracks(rng, oracle, F, cap, (), valid_share=0.8)
    match = RR.oracle_matcher(oracle, desc, t[10])
    ninl0 = rng.integers(10, 80, F - 1)
    assert (GR.states0(t, ninl0) == 2).all()
    compared = 0
    for solver in (_all_keyframes, GR.gate_solver):
        a, b = RR.sequential(t, match, solver, n_kf=n_kf, policy=policy), FQ.sequential(t, RR.adjacent(match), solver, n_kf=n_kf, policy=policy)
        assert not (b["state"] == 0).any() and np.array_equal(a["pred"], np.arange(F) - 1) and (a["gap"] == 1).all()
        for K in (0, 1, 2, F - 1):
            if K == 0:
                x, y = a, b
            else:
                x = RR.passes(t, match, solver, K, ninl0, n_kf=n_kf, policy=policy)
                y = FQ.passes(t, RR.adjacent(match), solver, K, ninl0, n_kf=n_kf, policy=policy)
                if any((u["state"] == 0).any() for u in y["per_pass"]):
                    continue
                for u, v in zip(x["per_pass"], y["per_pass"]):
                    assert np.array_equal(u["state"], v["state"]) and all(_same_item(i, j) for i, j in zip(u["items"], v["items"]))
                    assert np.array_equal(u["pred"], np.arange(F) - 1) and (u["gap"] == 1).all()
            compared += 1
            for k in ("G", "state", "kf_frame", "evicted", "n_kf"):
                assert np.array_equal(x[k], y[k]), (K, k)
            assert x["status"] == y["status"] and KR.same_windows(x["windows"], y["windows"], rtol=0, atol=0)
            assert len(x["tables"]) == len(y["tables"]) and all(np.array_equal(u, v) for u, v in zip(x["tables"], y["tables"]))
            assert len(x["feats"]) == len(y["feats"]) and all(np.array_equal(u, v) for u, v in zip(x["feats"], y["feats"]))
            assert all(_same_item(u, v) for u, v in zip(x["items"], y["items"]))
    assert compared >= 5, compared


def test_pairs_rule():
    """the pairing on hand-made state vectors: runs of 10 and 11, a state vector that already holds 3s, a rejected frame directly after frame 0"""
    st = np.array([2, 0, 1, 0, 0, 2], np.int32)
    pred, gap, eff = RR.pairs(st)
    assert pred.tolist() == [-1, 0, 0, 2, 2, 2] and gap.tolist() == [1, 2, 1, 2, 3] and np.array_equal(eff, st)
    st = np.array([2, 1] + [0] * 10 + [2, 1], np.int32)
    pred, gap, eff = RR.pairs(st)
    assert pred[12] == 1 and gap[11] == 11 and pred[13] == 12 and not (eff == 3).any()
    st = np.array([2, 1] + [0] * 11 + [2, 1], np.int32)
    pred, gap, eff = RR.pairs(st)
    assert pred[12] == 1 and gap[11] == 11 and pred[13] == -1 and pred[14] == -1 and gap[12] == 1 and eff[13:].tolist() == [3, 3] and (eff[:13] == st[:13]).all()
    assert np.array_equal(RR.pairs(eff)[0], pred) and np.array_equal(RR.pairs(eff)[2], eff)   # (idempotent on its own output)
    assert RR.fallback_frames(pred).tolist() == [0, 0] + [1] * 13


def planted_case(oracle, pattern, cap=256):
    """(F, tables, descriptors, match, solver (a), stage-A counts, n_kf, policy) of a pattern -- shared with tests/test_gpu_recover.py"""
    F, rejected = PATTERNS[pattern]
    idx = sorted(PATTERNS).index(pattern)
    rng = np.random.default_rng(7200 + idx)
    t, desc = recover_tracks(rng, oracle, F, cap, rejected, valid_share=0.6)
    return F, t, desc, RR.oracle_matcher(oracle, desc, t[10]), planted_solver(rejected), rng.integers(10, 200, F - 1), 4, idx % 2


def check_planted_guards(oracle, pattern, t, desc, s):
    """what keeps a planted case from being vacuous, on the restatement's sequential result: exactly the planted frames rejected, an accepted frame
    at gap >= 2 whose wider gate admits a match that gap 1 refuses, the run of ten recovered at gap 11, the run of eleven Lost"""
    F, rejected = PATTERNS[pattern]
    lost = np.flatnonzero(s["state"] == 3)
    live = [f for f in range(1, F) if f not in lost]
    assert [f for f in live if s["state"][f] == 0] == [f for f in rejected if f not in lost], s["state"]
    assert any(s["gap"][f - 1] >= 2 and s["state"][f] in (1, 2) for f in live) or pattern == "run11", (s["state"], s["gap"])
    assert gap_matters(oracle, desc, t[10], s) > 0
    if pattern == "run10":
        assert s["gap"].max() == 11 and s["state"][12] in (1, 2) and len(lost) == 0 and not s["status"] & 8
    if pattern == "run11":
        assert lost.tolist() == [13, 14] and s["status"] & 8 and (s["pred"][13:] == -1).all() and np.array_equal(s["G"][13], s["G"][1])
        assert all(w == {} for w in s["windows"][13:]) and all(len(x) == 0 for x in s["tables"][12:])


def test_passes_reproduce_the_sequential_loop_planted(oracle):
    """solver (a): exactly the planted frames are rejected; contract (B) for K = 1 .. F - 1 on every pattern; states 0, 1, 2 and 3 all occur"""
    states = set()
    for pattern in sorted(PATTERNS):
        F, t, desc, match, solver, ninl0, n_kf, policy = planted_case(oracle, pattern)
        s = RR.sequential(t, match, solver, n_kf=n_kf, policy=policy)
        check_planted_guards(oracle, pattern, t, desc, s)
        states |= set(s["state"].tolist())
        for K in range(1, F):
            check_contract_b(RR.passes(t, match, solver, K, ninl0, n_kf=n_kf, policy=policy), s, K, F, pattern)
    assert states == {0, 1, 2, 3}, states


@pytest.mark.parametrize("seed", range(2))
def test_passes_reproduce_the_sequential_loop_count_solver(oracle, seed):
    """solver (b): rejections that hang on the input count, so that the states change between passes; contract (B) for K = 1 .. F - 1.
    Thresholds were chosen on this restatement alone so that the guards hold (seed 0: 100, seed 1: 110)."""
    rng = np.random.default_rng(7300 + seed)
    F, cap, n_kf = 10, 256, 5
    t, desc = recover_tracks(rng, oracle, F, cap, (3, 6, 7), valid_share=0.5)
    match, solver = RR.oracle_matcher(oracle, desc, t[10]), count_solver((100, 110)[seed])
    ninl0 = rng.integers(0, 200, F - 1)
    s = RR.sequential(t, match, solver, n_kf=n_kf, policy=seed % 2)
    assert {0, 1, 2} <= set(s["state"].tolist()) or {0, 2} <= set(s["state"].tolist()), s["state"]
    changed = 0
    prev = None
    for K in range(1, F):
        p = RR.passes(t, match, solver, K, ninl0, n_kf=n_kf, policy=seed % 2)
        check_contract_b(p, s, K, F, seed)
        if prev is not None:
            changed += int(not np.array_equal(prev, p["state"]))
        prev = p["state"]
    assert changed > 0 and (s["state"] == 0).any() and any(s["gap"][f - 1] >= 2 and s["state"][f] != 0 for f in range(1, F)), (s["state"], s["gap"])


def test_header_and_signature_table_declare_the_new_entries(pkg):
    hdr = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = pkg.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in pkg.SIGNATURES and name in pkg.ABI_SYMBOLS and hasattr(lib, name), name
        assert hasattr(pkg.VO, name[len("vslam_"):]), name
    names = lib.vslam_kernel_names().decode().split()
    assert "frame_pairs_kernel" in names and "kf_gate_pairs_kernel" in names
    assert "BA results are not fed back" in hdr and "windows are independent" in hdr


@pytest.mark.parametrize("kw", [dict(f2f_queries="all"), dict(keyframe_gate=False, f2f_queries="all"), dict(keyframe_gate=True, pose_inputs="own_depth", f2f_queries="all"),
                                dict(pose_inputs="own_depth", keyframe_gate=False, f2f_queries="all"), dict(rejected_frames="drop"), dict(rejected_frames=True)])
def test_pipeline_refuses_recover_outside_feature_queries(kw):
    """rejected_frames="recover" needs pose_inputs="map", keyframe_gate="per_pass" and f2f_queries="features"; unknown values are refused -- all before
    any device work"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    args = dict(ba_windows="tracks", pose_inputs="map", pose_passes=1, keyframe_gate="per_pass", f2f_queries="features", rejected_frames="recover")
    args.update(kw)
    with pytest.raises(AssertionError):
        KeyframePipeline(4, **args)
