"""GPU: KeyframePipeline.reobserve() and full_ba(reobserved=...) on the 20 + 5-frame scene and settings of tests/test_gpu_loop_closures.py, one step for
the whole module: the device's matches against the yardstick on the arrays pulled from the pipeline, what the new observations and merges do to the
full BA problem, the precision of the applied matches against the render depth and poses, the full BA on the new problem against its yardstick,
and full_ba() without the argument unchanged."""
import time

import numpy as np
import pytest

import full_ba_cases as Cs
import full_ba_ref as FR
import place_inputs as PI
import project_match_ref as PR
import project_match_truth as PT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(synth):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    inputs = PI.loop_inputs(synth)
    pipe = KeyframePipeline(25, anms_num=500, n_kf=5, unique_frames=20, depth="sgbm", ba_windows="tracks", segments=[20, 5],
                            segment_sequences=[inputs["A"] + inputs["B"], inputs["foreign"]], landmark_ids=True)
    try:
        t0 = time.perf_counter()
        pipe.step(); pipe.vo.sync()
        t_step = time.perf_counter() - t0
        db = pipe.vo.place_db(rows=500, capacity=64)
        edges = pipe.loop_closures(db, min_gap=10, min_score=60, K=3, seq_ids=[0, 0])
        corrected = pipe.close_loops(edges)
        plain = pipe.full_ba(edges, poses=corrected); plain_fba = pipe.full_ba_result
        t0 = time.perf_counter()
        reobs = pipe.reobserve(edges)
        t_reobs = time.perf_counter() - t0
        again = pipe.full_ba(edges, poses=corrected); again_fba = pipe.full_ba_result
        fused = pipe.full_ba(edges, poses=corrected, reobserved=reobs); fused_fba = pipe.full_ba_result
        print("step %.1f ms, reobserve() %.1f ms of which the device call %.2f ms" % (t_step * 1e3, t_reobs * 1e3, pipe.project_match_ms))
        o = pipe.download()
        yield dict(pipe=pipe, inputs=inputs, edges=edges, corrected=corrected, plain=plain, plain_fba=plain_fba, again=again, again_fba=again_fba, reobs=reobs,
                   fused=fused, fused_fba=fused_fba, out=o, batch=pipe.project_match_batch, result=pipe.project_match_result)
    finally:
        pipe.close()


def test_matches_equal_the_yardstick(run, pkg):
    pipe, b, o = run["pipe"], run["batch"], run["out"]
    B, cap = pipe.B, pipe.cap
    kps = pipe.d_kps[:B].cpu().numpy().view(np.float32).reshape(B, cap, 7)[:, :, :2]
    desc = pipe.d_desc[:B].cpu().numpy(); n = pipe.d_cnt[:B].cpu().numpy()
    p = pipe.vo.params
    want = PR.project_match(b["lm_off"], b["item_img"], b["item_T"], b["lm_xyz"], b["lm_desc_row"], desc.reshape(-1, 32), kps, desc, n, list(p.cam)[:4], p.img_w, p.img_h,
                            radius_px=15.0, tau=50, ratio_pct=80, z_min=p.depth_min, z_max=p.depth_max)
    got = run["result"]
    counts = np.bincount(got["status"], minlength=8)
    print("%d items, %d landmarks, status counts %s, candidates per landmark %.2f" % (len(b["item_img"]), len(b["lm_desc_row"]), dict(zip(PR.STATUS_NAMES, counts.tolist())),
                                                                                      got["n_cand"].mean()))
    for key in ("status", "match", "dist", "n_cand"):
        assert np.array_equal(got[key], want[key]), key
    assert counts[PR.MATCHED] > 100 and counts[PR.INVALID] == 0


def _per_landmark(fba):
    rep = fba["report"]
    return rep["observations"] / rep["landmarks"]


def test_observations_per_landmark_rise_and_a_loop_edge_merges(run):
    before, after = _per_landmark(run["plain_fba"]), _per_landmark(run["fused_fba"])
    rep, frep = run["reobs"]["report"], run["fused_fba"]["report"]
    print("observations per landmark %.4f -> %.4f (%d / %d -> %d / %d)" % (before, after, run["plain_fba"]["report"]["observations"], run["plain_fba"]["report"]["landmarks"],
                                                                          frep["observations"], frep["landmarks"]))
    print("reobserve report:", rep)
    print("full BA report:", frep)
    for s, (a, c) in enumerate(zip(run["plain_fba"]["segments"], run["fused_fba"]["segments"])):
        print("segment %d: LM / PCG iterations %d / %d without, %d / %d with; chi2 %.6e -> %.6e without, %.6e -> %.6e with"
              % (s, a["stats"]["lm_iters"], a["stats"]["pcg_iters"], c["stats"]["lm_iters"], c["stats"]["pcg_iters"], a["stats"]["chi2_init"], a["stats"]["chi2_final"],
                 c["stats"]["chi2_init"], c["stats"]["chi2_final"]))
    assert after > before
    assert rep["merges_loop"] >= 1
    assert frep["observations_reobserved"] == len(run["reobs"]["observations"]) == rep["observations_added"] and frep["landmarks_merged"] >= 1


def test_precision_of_the_applied_matches(run, synth):
    """every applied match (an added observation or a merge) against the render depth and poses: the landmark's creating keypoint and the keypoint it
    was given must be the same world point within max(0.05 m, 2 % of depth).  The bound is the CPU precision test's figure less 0.05: estimated poses
    and stereo depth replace render geometry here."""
    pipe, inputs = run["pipe"], run["inputs"]
    frames = inputs["A"] + inputs["B"] + inputs["foreign"]
    B, cap = pipe.B, pipe.cap
    kps = pipe.d_kps[:B].cpu().numpy().view(np.float32).reshape(B, cap, 7)[:, :, :2]
    K4 = list(pipe.vo.params.cam)[:4]
    for kind, name in ((None, "all"), (0, "local"), (1, "loop")):
        rows = np.concatenate([run["reobs"]["observations"], run["reobs"]["merging_matches"]])
        if kind is not None:
            rows = rows[rows["kind"] == kind]
        ok_n = judged = 0
        for r in rows:
            cf, ck = int(r["lm_id"]) // cap, int(r["lm_id"]) % cap
            Wa, _ = PT.world_points(kps[cf, ck], frames[cf][3], frames[cf][2], K4, synth.R_from_quat)
            Wb, z = PT.world_points(kps[int(r["frame"]), int(r["kp"])], frames[int(r["frame"])][3], frames[int(r["frame"])][2], K4, synth.R_from_quat)
            if np.isfinite(Wa).all() and np.isfinite(Wb).all():
                judged += 1; ok_n += int(PT.correct(Wa, Wb, z)[0])
        prec = ok_n / max(judged, 1)
        print("applied matches (%s): %d, judged %d, correct %d, precision %.4f (bound %.3f)" % (name, len(rows), judged, ok_n, prec, PT.CPU_PRECISION - 0.05))
        if kind is None:
            assert judged >= 0.9 * len(rows) and prec >= PT.CPU_PRECISION - 0.05


def test_full_ba_with_reobserved_against_its_yardstick(run):
    for s, seg in enumerate(run["fused_fba"]["segments"]):
        p, st = seg["problem"], seg["stats"]
        st0 = run["plain_fba"]["segments"][s]["stats"]
        print("segment %d: status %d, %d observations dropped (without the new observations: status %d, %d dropped)"
              % (s, st["status"], st["n_obs_dropped"], st0["status"], st0["n_obs_dropped"]))
        if st["n_obs_dropped"]:
            P = FR.camera_points(p["T"], p["X"], p)
            for o in np.flatnonzero(P[:, 2] <= 0):
                lid = seg["lm_id"][seg["in_problem"]][p["lm"][o]]
                print("  behind the camera at the input state: keyframe %d, landmark id %d (local %d, %d observations), Pz %.3f, disp %.2f"
                      % (p["kf"][o], lid, p["lm"][o], (p["lm"] == p["lm"][o]).sum(), P[o, 2], p["disp"][o]))
        assert st["status"] == 0, (s, st["status"])
        t0 = time.perf_counter()
        ref = FR.solve(p, **Cs.CONVERGED)
        T_dev = run["fused"][s][1]
        order = np.argsort(run["fused"][s][0], kind="stable")
        dT = np.abs(T_dev[order] - ref["T"]).max(); dX = np.abs(seg["xyz_problem"] - ref["X"]).max() if len(ref["X"]) else 0.0
        print("segment %d: %d keyframes, %d landmarks, %d observations; yardstick %.1f s; largest difference poses %.3e, points %.3e; chi2 %.9e device, %.9e yardstick"
              % (s, len(p["T"]), len(p["X"]), len(p["kf"]), time.perf_counter() - t0, dT, dX, st["chi2_final"], ref["chi2_final"]))
        assert np.allclose(T_dev[order], ref["T"], rtol=1e-4, atol=1e-6)
        assert np.allclose(seg["xyz_problem"], ref["X"], rtol=1e-4, atol=1e-6)


def test_full_ba_without_the_argument_is_unchanged(run):
    """the same call before and after reobserve(): the same problem arrays and the same bytes out"""
    for (ia, Ta), (ib, Tb) in zip(run["plain"], run["again"]):
        assert np.array_equal(ia, ib) and Ta.tobytes() == Tb.tobytes()
    assert run["plain_fba"]["report"] == run["again_fba"]["report"]
    for a, b in zip(run["plain_fba"]["segments"], run["again_fba"]["segments"]):
        for key in ("T", "X", "kf", "lm", "uv", "disp", "ei", "ej", "Z", "w"):
            assert a["problem"][key].tobytes() == b["problem"][key].tobytes(), key
        assert a["xyz"].tobytes() == b["xyz"].tobytes()
    assert "observations_reobserved" not in run["plain_fba"]["report"]
