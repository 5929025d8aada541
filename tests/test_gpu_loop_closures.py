"""GPU: KeyframePipeline.loop_closures on a rendered drive that revisits its places (tests/place_inputs.py): every revisit's first candidate is its
twin and is accepted, nothing else has a candidate, the integer columns equal the restatement on the pipeline's own descriptors, the verification
equals the oracle's matcher + RANSAC, the relative poses agree with the render poses, and a database carried over two steps finds the same loops."""
import numpy as np
import pytest

import place_inputs as PI
import place_ref as P

pytestmark = pytest.mark.gpu

MIN_GAP, MIN_SCORE, K, TAU = 10, 60, 3, 30   # 60 lies between the 54 and 83 measured on the oracle (place_inputs.py): conditions, not tolerances


@pytest.fixture(scope="module")
def inputs(synth):
    return PI.loop_inputs(synth)


@pytest.fixture(scope="module")
def one_step(inputs):
    """passes A and B as one segment of 20 frames, the foreign place as a second segment, all in the same sequence id so that the foreign frames
    are eligible against the drive (frames 20..24 against 0..14 at min_gap 10)"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    pipe = KeyframePipeline(25, anms_num=500, n_kf=5, unique_frames=20, depth="sgbm", ba_windows="tracks", segments=[20, 5],
                            segment_sequences=[inputs["A"] + inputs["B"], inputs["foreign"]])
    try:
        pipe.step()
        db = pipe.vo.place_db(rows=500, capacity=64)
        edges = pipe.loop_closures(db, min_gap=MIN_GAP, min_score=MIN_SCORE, K=K, seq_ids=[0, 0])
        o = pipe.download()
        yield dict(edges=edges, out=o, stats=db.stats())
    finally:
        pipe.close()


def test_every_revisit_finds_its_twin_and_nothing_else_has_a_candidate(one_step):
    e = one_step["edges"]
    assert one_step["stats"]["n_entries"] == 25 and one_step["stats"]["n_refused"] == 0
    first = {}
    for row in e:
        first.setdefault(int(row["entry_q"]), row)
    assert sorted(first) == list(range(10, 20)), sorted(first)          # no A frame (0..9) and no foreign frame (20..24) has a candidate
    for q, row in first.items():
        assert row["entry_c"] == q - 10 and row["frame_q"] == q and row["frame_c"] == q - 10 and row["seq"] == 0, row
        assert row["score"] >= MIN_SCORE and row["accepted"] and row["n_inliers"] >= 10, row
    assert (e["score"] >= MIN_SCORE).all() and (e["frame_c"] <= e["frame_q"] - MIN_GAP).all()


def test_integer_columns_equal_the_restatement(one_step):
    """score, candidates and their order from tests/place_ref.py fed with the pipeline's own downloaded descriptors"""
    o, e = one_step["out"], one_step["edges"]
    ref = P.PlaceRef(500, 64)
    ref.add([o["desc"][b] for b in range(25)], o["cnt"][:25], [0] * 25, list(range(25)))
    score = ref.score(0, 25, TAU, MIN_GAP)
    cand, cs = P.select(score, K, MIN_SCORE)
    want = [(q, int(cand[q, r]), int(cs[q, r])) for q in range(25) for r in range(K) if cand[q, r] >= 0]
    assert [(int(r["entry_q"]), int(r["entry_c"]), int(r["score"])) for r in e] == want
    twin = [int(score[10 + i, i]) for i in range(10)]
    other = max(int(np.delete(score[10 + i], i).max()) for i in range(10))
    print("twin scores %s, best other eligible %d, foreign best %d" % (twin, other, int(score[20:].max())))
    assert min(twin) >= MIN_SCORE > other and score[20:].max() < MIN_SCORE


def _pose_error(synth, T, T_true):
    """(translation error in metres, rotation error in radians)"""
    R, Rt = synth.R_from_quat(np.asarray(T[:4])), synth.R_from_quat(np.asarray(T_true[:4]))
    c = (np.trace(R @ Rt.T) - 1.0) / 2.0
    return float(np.linalg.norm(np.asarray(T[4:]) - np.asarray(T_true[4:]))), float(np.arccos(np.clip(c, -1.0, 1.0)))


def test_verification_equals_the_oracle_and_agrees_with_the_render_poses(one_step, inputs, oracle, synth):
    """Per edge: match and inlier counts equal the oracle's feature_matching + pnp_ransac on the same entries, the pose within the project's 1e-4
    parity rule.  Per twin edge: T_q_c against the render poses.  Measured on an MI355X run of this test: the oracle's own worst error on the ten pairs
    (its pnp_ransac on its own matches, no refinement) is 0.1004 m / 0.00337 rad, and the device's is the same to the digits shown; the device must
    stay within twice the oracle's, whatever it measures to in the run."""
    o, e = one_step["out"], one_step["edges"]
    poses = [f[2] for f in inputs["A"] + inputs["B"] + inputs["foreign"]]
    worst_oracle, worst_gpu = [0.0, 0.0], [0.0, 0.0]
    for row in e:
        q, c = int(row["entry_q"]), int(row["entry_c"])
        nq, nc = int(o["cnt"][q]), int(o["cnt"][c])
        sel = np.flatnonzero(o["valid"][c][:nc])
        om = oracle.feature_matching(np.ascontiguousarray(o["desc"][c][sel]), np.ascontiguousarray(o["desc"][q][:nq]), 1.0)
        assert row["n_matches"] == len(om), (q, c)
        if len(om) < 10:
            assert row["n_inliers"] == 0 and not row["accepted"]
            continue
        uv = np.stack([o["kps"][q]["x"], o["kps"][q]["y"]], 1)[om["trainIdx"]]
        wT, _, wn, _ = oracle.pnp_ransac(o["xyz"][c][sel[om["queryIdx"]]], uv)
        assert row["n_inliers"] == wn and row["accepted"] == (wn >= 10), (q, c, row["n_inliers"], wn)
        assert np.allclose(row["T_q_c"], wT, rtol=1e-4, atol=1e-6), (q, c)
        if c == q - 10:   # the twin: ground truth from the render poses, T_q_c = T_q_w o T_c_w^-1
            Rq, Rc = synth.R_from_quat(poses[q][:4]), synth.R_from_quat(poses[c][:4])
            T_true = synth.se3_from_Rt(Rq @ Rc.T, poses[q][4:] - Rq @ Rc.T @ poses[c][4:])
            for w_, T in ((worst_oracle, wT), (worst_gpu, row["T_q_c"])):
                et, er = _pose_error(synth, T, T_true)
                w_[0], w_[1] = max(w_[0], et), max(w_[1], er)
    print("worst error against the render poses: oracle %.4f m / %.5f rad, device %.4f m / %.5f rad" % (*worst_oracle, *worst_gpu))
    assert worst_oracle[0] > 0 and worst_gpu[0] <= 2 * worst_oracle[0] and worst_gpu[1] <= 2 * worst_oracle[1]


def test_a_database_carried_over_two_steps_finds_the_same_loops(one_step, inputs):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    pipe = KeyframePipeline(10, anms_num=500, unique_frames=10, depth="sgbm", with_ba=False, sequence=inputs["A"])
    try:
        db = pipe.vo.place_db(rows=500, capacity=32)
        pipe.step()
        e1 = pipe.loop_closures(db, min_gap=MIN_GAP, min_score=MIN_SCORE, K=K)
        assert len(e1) == 0 and len(db) == 10
        pipe.show_sequence(inputs["B"])
        pipe.step()
        e2 = pipe.loop_closures(db, min_gap=MIN_GAP, min_score=MIN_SCORE, K=K, frame_offset=10)
        assert len(db) == 20
    finally:
        pipe.close()
    want = one_step["edges"][one_step["edges"]["entry_q"] < 20]
    assert len(e2) == len(want) >= 10
    for f in ("entry_q", "entry_c", "seq", "frame_q", "frame_c", "score", "n_matches", "n_inliers", "accepted"):
        assert np.array_equal(e2[f], want[f]), f
    assert np.allclose(e2["T_q_c"], want["T_q_c"], rtol=1e-9, atol=1e-12)


def test_default_ping_pong_batch_scores_every_row_against_its_twin():
    """the default batch drives one rendered sequence forwards and backwards: a frame shown again is the same image, so every one of its rows has an
    exact duplicate in its twin and the score is its row count (depth="match": the points reach the database through the L/R table)"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    pipe = KeyframePipeline(6, anms_num=500, unique_frames=4, depth="match", with_ba=False, seed=3)
    try:
        assert pipe.frame_of == [0, 1, 2, 3, 2, 1]
        pipe.step()
        e = pipe.loop_closures(min_gap=2, min_score=MIN_SCORE, K=1)
        cnt = pipe.download()["cnt"]
    finally:
        pipe.close()
    twins = {int(r["entry_q"]): r for r in e}
    assert twins[4]["entry_c"] == 2 and twins[4]["score"] == cnt[4] and twins[5]["entry_c"] == 1 and twins[5]["score"] == cnt[5]
    for q in (4, 5):
        assert twins[q]["accepted"] and np.linalg.norm(twins[q]["T_q_c"][4:]) < 0.05 and abs(twins[q]["T_q_c"][3]) > 0.9999
