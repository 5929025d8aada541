"""GPU: full_ba_kernel (vslam_full_ba_dev) against the numpy yardstick of tests/full_ba_ref.py.  The reference has no such stage; the guards of the
yardstick and of every case run here are in tests/test_full_ba_ref.py."""
import numpy as np
import pytest

import full_ba_cases as Cs
import full_ba_ref as R

pytestmark = pytest.mark.gpu


def run(vo, problems, store=-1, batch=None, **params):
    """the problems as one batch through VO.full_ba; camera and Huber width are the first problem's (one camera per call)"""
    b = Cs.pack(problems) if batch is None else batch
    p0 = problems[0]
    vo.set_tuning(fba_store=store)
    try:
        return vo.full_ba(b["T"], b["X"], dict(kf=b["kf_off"], lm=b["lm_off"], obs=b["obs_off"], edge=b["edge_off"]),
                          dict(kf=b["kf"], lm=b["lm"], uv=b["uv"], disp=b["disp"], active=b["obs_active"]),
                          dict(i=b["ei"], j=b["ej"], Z=b["Z"], w=b["w"], active=b["edge_active"]), fixed=b["fixed"], K4=p0["K4"], bf=p0["bf"],
                          huber_delta=p0["huber"], **params)
    finally:
        vo.set_tuning(fba_store=-1)


def split(out, problems):
    """the per-problem slices (T, xyz, obs_chi2, stats record) of a batch result"""
    n = np.cumsum([0] + [len(p["T"]) for p in problems]); m = np.cumsum([0] + [len(p["X"]) for p in problems]); o = np.cumsum([0] + [len(p["kf"]) for p in problems])
    return [(out["T"][n[k]:n[k + 1]], out["xyz"][m[k]:m[k + 1]], out["obs_chi2"][o[k]:o[k + 1]], out["stats"][k]) for k in range(len(problems))]


def check_against_cost_and_gradient(p, T, X, st, label):
    """chi2_final is the cost numpy finds at the device's state (rtol 1e-9: reordering in f64), the exact gradient there is at most 1e-6 of the initial
    one, and the cost fell"""
    cost, gT, gX = R.cost_and_gradient(T, X, p)
    gn = float(np.sqrt((gT * gT).sum() + (gX * gX).sum()))
    g0 = Cs.gradient_norm(p, p["T"], p["X"])
    print("%s: chi2 %.9e -> %.9e (numpy at the device's state %.9e), gradient %.2e of initial, %d LM / %d PCG iterations, status %d"
          % (label, st["chi2_init"], st["chi2_final"], cost, gn / g0, st["lm_iters"], st["pcg_iters"], st["status"]))
    assert np.isclose(st["chi2_final"], cost, rtol=1e-9, atol=0)
    assert gn <= 1e-6 * g0
    assert st["chi2_final"] < st["chi2_init"]


def test_evaluation_only(vo):
    """max_iters = 0: chi2_init and the per-observation chi2 against numpy at rtol 1e-9, poses and points copied.  Mono and stereo observations, Huber
    on both branches and loop edges are all in the batch's first camera; a wrong convention shows at order one."""
    problems = [Cs.parity_cases()["arc_12_63"], Cs.parity_cases()["ring_5"], Cs.parity_cases()["arc_65_300"]]
    out = run(vo, problems, max_iters=0)
    for p, (T, X, chi2, st) in zip(problems, split(out, problems)):
        want = R.obs_chi2(p["T"], p["X"], p)
        assert want.min() > 1e-8
        assert np.array_equal(T, p["T"]) and np.array_equal(X, p["X"])
        assert np.allclose(chi2, want, rtol=1e-9, atol=0)
        assert np.isclose(st["chi2_init"], R.cost(p["T"], p["X"], p), rtol=1e-9, atol=0) and st["chi2_final"] == st["chi2_init"]
        assert (st["lm_iters"], st["pcg_iters"], st["status"], st["n_free"], st["n_obs_dropped"]) == (0, 0, 0, len(p["T"]) - 1, 0)
    assert (vo.full_ba_status(3) == 0).all()
    h = Cs.huber_case()
    T, X, chi2, st = split(run(vo, [h], max_iters=0), [h])[0]
    assert np.isclose(st["chi2_init"], R.cost(h["T"], h["X"], h), rtol=1e-9, atol=0) and st["chi2_init"] < 0.9 * chi2.sum()


@pytest.mark.parametrize("name", Cs.PARITY_NAMES)
def test_parity(vo, name):
    p, ref = Cs.reference(name)
    T, X, chi2, st = split(run(vo, [p]), [p])[0]
    check_against_cost_and_gradient(p, T, X, st, name)
    print("   max |dT| %.2e, max |dX| %.2e, chi2_final / yardstick - 1 = %.2e (yardstick's PCG mode: %d LM / %d PCG iterations)"
          % ((np.abs(T - ref["T"]).max(), np.abs(X - ref["X"]).max(), st["chi2_final"] / ref["chi2_final"] - 1) + _pcg_counts(name)))
    assert st["status"] == 0 and st["n_obs_dropped"] == 0 and st["n_free"] == int((~R.held_keyframes(p)).sum())
    assert np.isclose(st["chi2_init"], ref["chi2_init"], rtol=1e-9, atol=0)
    assert np.allclose(T, ref["T"], rtol=1e-4, atol=1e-6)
    assert np.allclose(X, ref["X"], rtol=1e-4, atol=1e-6)
    assert np.allclose(chi2, R.obs_chi2(T, X, p), rtol=1e-9, atol=1e-24)


def _pcg_counts(name):
    r = R.solve(Cs.parity_cases()[name], mode="pcg")
    return r["lm_iters"], r["pcg_iters"]


def test_recomputed_observations_give_the_same_answer(vo):
    """fba_store = 0 recomputes (P, B) in every conjugate-gradient phase: the same problem, the same bounds"""
    for name in ("arc_12_64_obs257", "huber", "ring_5"):
        p, ref = Cs.reference(name)
        T, X, chi2, st = split(run(vo, [p], store=0), [p])[0]
        check_against_cost_and_gradient(p, T, X, st, name + " recomputed")
        assert st["status"] == 0 and np.allclose(T, ref["T"], rtol=1e-4, atol=1e-6) and np.allclose(X, ref["X"], rtol=1e-4, atol=1e-6)


def test_the_inputs_matter(vo):
    """the device, as the yardstick (tests/test_full_ba_ref.py): without the Huber kernel, without the loop edges, without the disparities the answer
    moves by more than the parity tolerance"""
    far = lambda T, X, ref: not (np.allclose(T, ref["T"], rtol=1e-4, atol=1e-6) and np.allclose(X, ref["X"], rtol=1e-4, atol=1e-6))
    for name, q in (("huber", lambda p: Cs.without(p, huber=0.0)), ("ring_5", Cs.no_edges), ("arc_12_63", lambda p: Cs.without(p, disp=None))):
        p, ref = Cs.reference(name)
        q = q(p)
        T, X, _, st = split(run(vo, [q]), [q])[0]
        assert st["lm_iters"] > 0 and far(T, X, ref), name


def test_determinism_and_batching(vo):
    """three problems of different sizes: twice the same bytes, every problem bit for bit its output alone, under either form"""
    cases = Cs.parity_cases()
    problems = [cases["arc_2_64"], cases["ring_5"], cases["arc_65_65"]]
    for store in (1, 0):
        out = run(vo, problems, store)
        again = run(vo, problems, store)
        for k in ("T", "xyz", "obs_chi2", "stats"):
            assert out[k].tobytes() == again[k].tobytes(), k
        status = vo.full_ba_status(len(problems))
        assert np.array_equal(status, out["stats"]["status"]) and list(status) == [0, 0, 0]
        parts = split(out, problems)
        for k, p in enumerate(problems):
            alone = split(run(vo, [p], store), [p])[0]
            for a, b in zip(parts[k], alone):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (store, k)
            assert parts[k][3]["lm_iters"] > 0 and parts[k][3]["chi2_final"] < parts[k][3]["chi2_init"]


def test_bad_input_skips_or_passes_through_only_its_problem(vo, pkg):
    cases = Cs.parity_cases()
    problems = [cases["arc_12_63"], cases["ring_1"], cases["arc_12_65"]]
    b = Cs.pack(problems)
    good = run(vo, problems)
    alone = [split(run(vo, [p]), [p])[0] for p in problems]
    n, m, o = b["kf_off"], b["lm_off"], b["obs_off"]

    def neighbours_untouched(out, skip):
        for k, part in enumerate(split(out, problems)):
            if k not in skip:
                for x, y in zip(part, alone[k]):
                    assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), k

    # problem 1 claims more observations than its range holds: its end offset lies past problem 2's start; both are skipped entirely
    bad = dict(b, obs_off=b["obs_off"].copy()); bad["obs_off"][2] = b["obs_off"][3] + 1
    out = run(vo, problems, batch=bad)
    assert list(out["stats"]["status"]) == [0, pkg.FBA_BAD_INDEX, pkg.FBA_BAD_INDEX]
    assert out["T"][:n[1]].tobytes() == good["T"][:n[1]].tobytes() and (out["T"][n[1]:] == 0).all() and (out["xyz"][m[1]:] == 0).all()
    # offsets out of order: problem 0's end lies past problem 1's end, inside problem 2's range, so none of the three ranges is its own
    bad = dict(b, lm_off=b["lm_off"].copy()); bad["lm_off"][1] = b["lm_off"][2] + 3
    out = run(vo, problems, batch=bad)
    assert list(out["stats"]["status"]) == [pkg.FBA_BAD_INDEX] * 3 and (out["T"] == 0).all() and (out["xyz"] == 0).all()
    # ... and a negative first offset fails problem 0 alone
    bad = dict(b, edge_off=b["edge_off"].copy()); bad["edge_off"][0] = -1
    out = run(vo, problems, batch=bad)
    assert list(out["stats"]["status"]) == [pkg.FBA_BAD_INDEX, 0, 0]
    neighbours_untouched(out, {0})
    # a keyframe id, a landmark id out of range, observations not sorted by landmark, an edge between a keyframe and itself: passed through
    for key, at, value in (("kf", o[1] + 5, n[2] - n[1]), ("lm", o[1] + 5, -1), ("lm", o[1] + 5, m[2] - m[1] - 1), ("ej", 0, b["ei"][0])):
        bad = dict(b, **{key: b[key].copy()}); bad[key][at] = value
        out = run(vo, problems, batch=bad)
        assert list(out["stats"]["status"]) == [0, pkg.FBA_BAD_INDEX, 0], (key, value)
        assert np.array_equal(out["T"][n[1]:n[2]], b["T"][n[1]:n[2]]) and np.array_equal(out["xyz"][m[1]:m[2]], b["X"][m[1]:m[2]])
        assert out["stats"][1]["lm_iters"] == 0
        neighbours_untouched(out, {1})
    # non-finite values: a pose, a point, a pixel, an infinite disparity, a measurement, and a negative weight
    for key, at, value in (("T", (n[1] + 3, 5), np.nan), ("X", (m[1] + 2, 0), np.inf), ("uv", (o[1] + 7, 1), np.nan), ("disp", o[1] + 7, np.inf), ("Z", (0, 2), np.nan),
                           ("w", (0, 0), -1.0)):
        bad = dict(b, **{key: b[key].copy()}); bad[key][at] = value
        out = run(vo, problems, batch=bad)
        assert list(out["stats"]["status"]) == [0, pkg.FBA_NONFINITE, 0], (key, value)
        assert np.array_equal(out["xyz"][m[1]:m[2]], bad["X"][m[1]:m[2]], equal_nan=True) and out["stats"][1]["lm_iters"] == 0
        neighbours_untouched(out, {1})


def test_degenerate_problems(vo):
    for name, (p, n_free, status, dropped) in Cs.degenerate().items():
        T, X, chi2, st = split(run(vo, [p]), [p])[0]
        ref = R.solve(p)
        print("%s: chi2 %.6e -> %.6e (yardstick %.6e), %d LM iterations, status %d, %d dropped" % (name, st["chi2_init"], st["chi2_final"], ref["chi2_final"], st["lm_iters"], st["status"], st["n_obs_dropped"]))
        assert (st["status"], st["n_free"], st["n_obs_dropped"]) == (status, n_free, dropped), name
        assert np.isfinite(T).all() and np.isfinite(X).all() and np.isfinite(chi2).all() and np.isfinite(st["chi2_final"]), name
        assert np.isclose(st["chi2_init"], ref["chi2_init"], rtol=1e-9, atol=1e-24), name
        assert st["chi2_final"] <= st["chi2_init"], name
        if n_free == 0:
            assert np.array_equal(T, p["T"]), name
        if name in ("no_observations", "all_weights_zero"):
            assert np.array_equal(X, p["X"]) and np.array_equal(T, p["T"]), name
        if name in ("all_held", "one_keyframe"):   # structure only: every landmark moves to its triangulation
            assert st["lm_iters"] > 0 and st["chi2_final"] < st["chi2_init"] and np.isclose(st["chi2_final"], ref["chi2_final"], rtol=1e-6), name
        if name == "keyframe_without_observations":
            assert np.array_equal(T[5], p["T"][5]) and not np.array_equal(T[6], p["T"][6]), name
        if name == "observation_behind_camera":   # the landmark whose observations were all dropped is copied through
            assert np.array_equal(X[7], p["X"][7]) and st["chi2_final"] < st["chi2_init"], name
        if name == "single_stereo_landmark":   # three rows, three unknowns: the observation is met exactly
            assert chi2[-1] < 1e-12, name


def test_state_is_counted_in_device_bytes(pkg):
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        before = ctx.device_bytes
        p = Cs.parity_cases()["arc_65_300"]
        run(ctx, [p], max_iters=1)
        # 17 doubles per observation, 24 per landmark, 136 per keyframe, at the least
        assert ctx.device_bytes - before >= (len(p["kf"]) * 17 + 300 * 24 + 65 * 136) * 8
        with pytest.raises(pkg.VslamError):
            ctx.full_ba_status(2)   # (the last call had one problem)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the pipeline: step -> loop_closures -> close_loops -> full_ba
@pytest.fixture(scope="module")
def adjusted(synth):
    """the 20 + 5-frame scene of tests/place_inputs.py as the `closed` fixture of tests/test_gpu_pose_graph.py builds it, plus landmark_ids=True, through
    step(), loop_closures(), close_loops() and full_ba().  No accuracy claim against the render poses is made: see that fixture's docstring."""
    import place_inputs as PI
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    inputs = PI.loop_inputs(synth)
    pipe = KeyframePipeline(25, anms_num=500, n_kf=5, unique_frames=20, depth="sgbm", ba_windows="tracks", segments=[20, 5],
                            segment_sequences=[inputs["A"] + inputs["B"], inputs["foreign"]], landmark_ids=True)
    try:
        pipe.step()
        db = pipe.vo.place_db(rows=500, capacity=64)
        edges = pipe.loop_closures(db, min_gap=10, min_score=60, K=3, seq_ids=[0, 0])
        before = pipe.trajectories()
        corrected = pipe.close_loops(edges)
        result = pipe.full_ba(edges, poses=corrected)
        yield dict(pipe=pipe, edges=edges, before=before, corrected=corrected, result=result, fba=pipe.full_ba_result)
    finally:
        pipe.close()


def test_pipeline_full_ba_meets_the_bounds_on_the_problem_it_built(adjusted):
    fba, pipe = adjusted["fba"], adjusted["pipe"]
    rep = fba["report"]
    print("report:", rep)
    assert rep["edges_added"] >= 10 and rep["edges_added"] + rep["edges_not_accepted"] + rep["edges_unknown_seq"] + rep["edges_unknown_frame"] == len(adjusted["edges"])
    assert rep["observations_seen"] == rep["observations"] + rep["observations_duplicate"] + rep["observations_other_segment"] + rep["observations_dropped"]
    assert rep["landmarks_seen"] == rep["landmarks"] + rep["landmarks_dropped"]
    seen = set()
    for s, seg in enumerate(fba["segments"]):
        ids, T_dev = adjusted["result"][s]
        assert np.array_equal(ids, adjusted["before"][s][0]) and np.array_equal(ids, adjusted["corrected"][s][0])
        p, st = seg["problem"], seg["stats"]
        assert np.array_equal(p["T"], adjusted["corrected"][s][1]) and len(p["kf"]) > 50
        check_against_cost_and_gradient(p, T_dev, seg["xyz_problem"], st, "pipeline segment %d" % s)
        assert st["status"] & ~R.FBA_DROPPED == 0
        assert len(np.unique(seg["lm_id"])) == len(seg["lm_id"]) and len(seg["xyz"]) == len(seg["lm_id"]) and np.isfinite(seg["xyz"]).all()
        seen |= set(seg["lm_id"].tolist())
    assert seen == set(np.unique(pipe.window_landmark_ids()).tolist())
    assert sum(len(seg["lm_id"]) for seg in fba["segments"]) == len(seen)


def test_dense_map_takes_the_result(adjusted):
    pipe = adjusted["pipe"]
    a = pipe.dense_map(voxel_size=0.5, log2_capacity=20, step=4, poses=adjusted["corrected"]).extract()
    b = pipe.dense_map(voxel_size=0.5, log2_capacity=20, step=4, poses=adjusted["result"]).extract()
    assert len(a) > 0 and len(b) > 0 and (len(a) != len(b) or not np.array_equal(a, b))


def test_full_ba_needs_landmark_ids(synth):
    import place_inputs as PI
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    inputs = PI.loop_inputs(synth)
    pipe = KeyframePipeline(5, anms_num=500, n_kf=5, unique_frames=5, depth="sgbm", ba_windows="tracks", sequence=inputs["A"][:5])
    try:
        pipe.step()
        with pytest.raises(ValueError, match="landmark_ids"):
            pipe.full_ba()
    finally:
        pipe.close()
