"""The BA kernels -- lm_window_kernel, ba_resident_kernel in both widths, pose_only_wave_kernel in both forms -- on windows whose graph is degenerate
(tests/ba_topology_cases.py; their structure and the oracle's behaviour on them are pinned on the CPU by tests/test_ba_topology_cases.py), against the
CPU oracle at the tolerances of tests/test_gpu_lm.py and against recompute_chi2, a numpy f64 evaluation of the reference's edge that shares no code
with the oracle.

The per-edge chi2 an optimiser hands out is that of the last trial it evaluated (g2o's e->chi2() after optimize(), the oracle and the kernels alike),
the state that of the last accepted trial: the two belong together when the last iteration ended in an accepted trial.  The recomputation check
therefore reads the run's own record and, where the last iteration did not accept, repeats the call with the iteration count cut to the last
accepting one -- the kernels are deterministic, so that is the same trajectory, ending in an accepted trial.

Every test prints its figures (largest pose difference from the oracle, largest chi2 recomputation difference next to its allowance) before asserting."""
import numpy as np
import pytest

import ba_topology_cases as C
from test_gpu_lm import RTOL, _stats_close

pytestmark = pytest.mark.gpu
KF_MAX = 12
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
HOST = [n for n in C.case_names() if n not in C.HOST_ONLY_SKIP]
MAP_FORMS = {"general": dict(ba_resident=0), "resident256": dict(ba_resident=1, ba_lanes=256), "resident512": dict(ba_resident=1, ba_lanes=512)}
PO_FORMS = {"po_window0": dict(pose_only_window=0), "po_window1": dict(pose_only_window=1)}
KEYS = ("ba_resident", "ba_lanes", "pose_only_window", "pose_only_waves")


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.VO(device=0, max_batch=1)
    try:
        yield c
    finally:
        c.set_tuning(**{k: -1 for k in KEYS})
        c.close()


@pytest.fixture(scope="module")
def ref(oracle, cases):
    """the oracle's answers, once per case: local_ba and pose_only_window at 8 iterations"""
    out = {}
    for n in HOST:
        c = cases[n]
        out[n] = dict(map=oracle.local_ba(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], iters=8, update_poses=True, update_lms=True),
                      po=oracle.pose_only_window(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], iters=8))
    return out


_runs = {}


def _run(ctx, cases, name, form, iters=8):
    """one host-tier call, memoised: the oracle comparison and the recomputation check read the same run"""
    key = (name, form, iters)
    if key not in _runs:
        c = cases[name]
        tune = MAP_FORMS.get(form) or PO_FORMS[form]
        try:
            ctx.set_tuning(**tune)
            if form in MAP_FORMS:
                _runs[key] = ctx.optimize_map(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], True, True, iters)
            else:
                _runs[key] = ctx.optimize_pose_only(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], True, iters)
        finally:
            ctx.set_tuning(**{k: -1 for k in tune})
    return _runs[key]


def _stats_close_above_floor(g, w, c):
    """_stats_close of tests/test_gpu_lm.py on the iterations that START above the f64 evaluation floor of the cost (C.chi2_floor).  _stats_close
    counts an iteration as significant by its RELATIVE chi2 decrease; a window whose residuals can all be driven to zero (one edge: 2 residuals, 6 or
    9 unknowns) goes on 'decreasing' from 3e-26 to 1e-26 px^2, i.e. inside the rounding of one residual evaluation, where the sign of the gain ratio is
    noise.  The cut is taken on the ORACLE's record and applied to both; on every window with a non-zero optimum it removes nothing."""
    floor = C.chi2_floor(c["uv"])
    starts = [w["chi2_init"]] + list(w["chi2_iter"][:-1])
    n = 0
    while n < len(starts) and starts[n] > floor:
        n += 1
    cut = lambda s: dict(s, chi2_iter=s["chi2_iter"][:n], lambda_iter=s["lambda_iter"][:n], trials_iter=s["trials_iter"][:n])
    _stats_close(cut(g), cut(w))
    return n


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _untouched_parts(c, name, r, with_lms):
    n_lm = len(c["xyz"])
    unobserved = np.bincount(c["lm_idx"], minlength=n_lm) == 0
    if with_lms:
        assert _same_bits(r["xyz"][unobserved], c["xyz"][unobserved])                                 # landmarks nobody observes come back bit for bit ...
    assert (r["lm_inlier"][unobserved] == 1).all()                                                     # ... and no edge writes their flag
    if name in C.EMPTY_KF:
        k = C.EMPTY_KF[name]
        assert _same_bits(r["T"][k], c["T0"][k]), (r["T"][k] - c["T0"][k])                             # nothing pulls on the edgeless keyframe
        assert not np.array_equal(np.delete(r["T"], k, 0), np.delete(c["T0"], k, 0))


def _zero_edges(c, r):
    assert _same_bits(r["T"], c["T0"]) and _same_bits(r["xyz"], c["xyz"]) and (r["lm_inlier"] == 1).all() and len(r["chi2"]) == 0


# ------------------------------------------------------------------------------------------------ host tier, optimize_map
@pytest.mark.parametrize("form", list(MAP_FORMS))
@pytest.mark.parametrize("name", HOST)
def test_optimize_map_matches_the_oracle(ctx, oracle, cases, ref, name, form):
    c = cases[name]
    r = _run(ctx, cases, name, form)
    if name == "zero_edges":
        return _zero_edges(c, r)
    T, xyz, chi2, st = ref[name]["map"]
    print("TOPO map %-24s %-12s pose diff %.3e  xyz diff %.3e  chi2 diff %.3e" % (name, form, np.abs(r["T"] - T).max(), np.abs(r["xyz"] - xyz).max(), np.abs(r["chi2"] - chi2).max()))
    _stats_close_above_floor(r["stats"], st, c)
    assert np.allclose(r["T"], T, rtol=RTOL, atol=1e-6), np.abs(r["T"] - T).max()
    assert np.allclose(r["xyz"], xyz, rtol=RTOL, atol=1e-4), np.abs(r["xyz"] - xyz).max()
    assert np.allclose(r["chi2"], chi2, rtol=1e-4, atol=1e-6), np.abs(r["chi2"] - chi2).max()
    th, inl, _, _ = oracle.chi2_classify(chi2, c["lm_idx"], np.ones(len(c["xyz"]), np.uint8))
    assert r["threshold"] == th and np.array_equal(r["lm_inlier"], inl)
    _untouched_parts(c, name, r, True)


@pytest.mark.parametrize("name", HOST)
def test_resident_widths_give_the_same_bits(ctx, cases, name):
    a, b = _run(ctx, cases, name, "resident256"), _run(ctx, cases, name, "resident512")
    for k in ("T", "xyz", "chi2", "lm_inlier"):
        assert _same_bits(a[k], b[k]), k
    assert a["threshold"] == b["threshold"] and a["stats"] == b["stats"]


# ------------------------------------------------------------------------------------------------ host tier, optimize_pose_only
@pytest.mark.parametrize("form", list(PO_FORMS))
@pytest.mark.parametrize("name", HOST)
def test_optimize_pose_only_matches_the_oracle(ctx, oracle, cases, ref, name, form):
    c = cases[name]
    r = _run(ctx, cases, name, form)
    if name == "zero_edges":
        return _zero_edges(c, r)
    T, chi2, st = ref[name]["po"]
    print("TOPO po  %-24s %-12s pose diff %.3e  chi2 diff %.3e" % (name, form, np.abs(r["T"] - T).max(), np.abs(r["chi2"] - chi2).max()))
    assert np.allclose(r["T"], T, rtol=RTOL, atol=1e-7), np.abs(r["T"] - T).max()
    assert np.allclose(r["chi2"], chi2, rtol=1e-6, atol=1e-9), np.abs(r["chi2"] - chi2).max()
    _stats_close_above_floor(r["stats"], st, c)
    th, inl, _, _ = oracle.chi2_classify(chi2, c["lm_idx"], np.ones(len(c["xyz"]), np.uint8))
    assert r["threshold"] == th and np.array_equal(r["lm_inlier"], inl)
    assert _same_bits(r["xyz"], c["xyz"])
    _untouched_parts(c, name, r, False)


# ------------------------------------------------------------------------------------------------ the cost, recomputed without the oracle
def _accepted_run(ctx, cases, name, form):
    r = _run(ctx, cases, name, form)
    n = C.last_accepted_iteration(r["stats"])
    assert n >= 1, r["stats"]
    if n < r["stats"]["iterations"]:
        r2 = _run(ctx, cases, name, form, iters=n)
        assert r2["stats"]["chi2_iter"] == r["stats"]["chi2_iter"][:n]                               # the same trajectory, cut
        r = r2
    return r


@pytest.mark.parametrize("form", list(PO_FORMS))
@pytest.mark.parametrize("name", [n for n in HOST if n != "zero_edges"])
def test_pose_only_chi2_is_the_cost_of_the_returned_state(ctx, cases, name, form):
    """the state is exact (poses f64, landmarks the f32 input): 1e-9 relative plus 1e-12, where tests/test_gpu_jacobians.py holds the device residual"""
    c = cases[name]
    r = _accepted_run(ctx, cases, name, form)
    mine, total = C.recompute_chi2(r["T"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"])
    first, total0 = C.recompute_chi2(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"])
    diff = np.abs(mine - r["chi2"])
    print("TOPO po  %-24s %-12s recomputed chi2: largest diff %.3e (relative %.3e)  cost %.6g -> %.6g" % (name, form, diff.max(), (diff / np.maximum(mine, 1e-300)).max(), total0, total))
    assert np.allclose(r["chi2"], mine, rtol=1e-9, atol=1e-12), diff.max()
    assert np.isclose(total0, r["stats"]["chi2_init"], rtol=1e-9)
    assert total <= total0
    assert np.isclose(total, r["stats"]["chi2_final"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("form", list(MAP_FORMS))
@pytest.mark.parametrize("name", [n for n in HOST if n != "zero_edges"])
def test_optimize_map_chi2_is_the_cost_of_the_returned_state(ctx, cases, name, form):
    """the kernel evaluates at f64 landmark positions and stores f32: per edge, the allowance of C.f32_storage_allowance (derived there)"""
    c = cases[name]
    r = _accepted_run(ctx, cases, name, form)
    mine, total = C.recompute_chi2(r["T"], r["xyz"], c["kf_idx"], c["lm_idx"], c["uv"])
    first, total0 = C.recompute_chi2(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"])
    allow = C.f32_storage_allowance(r["T"], r["xyz"], c["kf_idx"], c["lm_idx"], c["uv"])
    diff = np.abs(mine - r["chi2"])
    worst = int(np.argmax(diff - allow))
    msg = "largest allowance %.3e, largest diff %.3e; closest edge %d: diff %.3e of %.3e allowed" % (allow.max(), diff.max(), worst, diff[worst], allow[worst])
    print("TOPO map %-24s %-12s recomputed chi2: %s  cost %.6g -> %.6g" % (name, form, msg, total0, total))
    assert (diff <= allow).all(), msg
    assert np.isclose(total0, r["stats"]["chi2_init"], rtol=1e-9)
    assert total <= total0


# ------------------------------------------------------------------------------------------------ the batched schedule
def _batch(pkg, ctx, wins, tune):
    """vslam_ba_batch_dev(schedule = 1) on the windows, stride 12 with per-window keyframe counts (as _run of tests/test_gpu_pose_only_forms.py)"""
    import torch
    d = "cuda"
    n = len(wins)
    lm_off = np.cumsum([0] + [len(w["xyz"]) for w in wins]).astype(np.int32)
    e_off = np.cumsum([0] + [len(w["kf_idx"]) for w in wins]).astype(np.int32)
    T0 = np.tile(IDENT, (n, KF_MAX, 1))
    inl0 = np.ones(int(lm_off[-1]), np.uint8)
    for i, w in enumerate(wins):
        T0[i, :w["n_kf"]] = w["T0"]
        if w.get("inl0") is not None:
            inl0[lm_off[i]:lm_off[i + 1]] = w["inl0"]
    T = torch.from_numpy(T0).to(d)
    xyz = torch.from_numpy(np.concatenate([w["xyz"] for w in wins])).to(d)
    kf = torch.from_numpy(np.concatenate([w["kf_idx"] for w in wins])).to(d)
    lm = torch.from_numpy(np.concatenate([w["lm_idx"] for w in wins])).to(d)
    uv = torch.from_numpy(np.concatenate([w["uv"] for w in wins])).to(d)
    inl = torch.from_numpy(inl0).to(d)
    chi = torch.zeros(int(e_off[-1]), dtype=torch.float64, device=d)
    nkf = torch.from_numpy(np.array([w["n_kf"] for w in wins], np.int32)).to(d)
    t_lm, t_e = torch.from_numpy(lm_off).to(d), torch.from_numpy(e_off).to(d)
    bb = pkg.BaBatch()
    bb.n_windows = n; bb.n_kf = KF_MAX
    bb.d_lm_off = t_lm.data_ptr(); bb.d_edge_off = t_e.data_ptr(); bb.d_T_c_w = T.data_ptr(); bb.d_xyz = xyz.data_ptr()
    bb.d_reliable = None; bb.d_lm_inlier = inl.data_ptr(); bb.d_kf_idx = kf.data_ptr(); bb.d_lm_idx = lm.data_ptr(); bb.d_uv = uv.data_ptr()
    bb.d_chi2 = chi.data_ptr(); bb.d_stats = None; bb.total_lm = int(lm_off[-1]); bb.total_edge = int(e_off[-1])
    bb.d_n_kf = nkf.data_ptr()
    try:
        ctx.set_tuning(**tune)
        torch.cuda.synchronize()
        ctx.ba_batch_dev(bb, schedule=1)
        ctx.sync()
        status = ctx.ba_status(n)
    finally:
        ctx.set_tuning(**{k: -1 for k in tune})
    return dict(T=T.cpu().numpy(), inl=inl.cpu().numpy(), status=status, T0=T0, inl0=inl0, lm_off=lm_off)


@pytest.fixture(scope="module")
def schedule_ref(oracle, cases):
    return {n: C.oracle_schedule(oracle, cases[n]) for n in cases}


@pytest.mark.parametrize("waves", [12, 4])
@pytest.mark.parametrize("resident", [0, 1])
def test_batched_schedule_matches_the_oracle_window_by_window(pkg, ctx, cases, schedule_ref, resident, waves):
    """a normal window, every case, a normal window, in one launch: each window against the oracle's composite schedule, the normal windows
    bit-identical to a launch that holds only the two of them, and the windows without an active edge untouched"""
    tune = dict(ba_resident=resident, pose_only_waves=waves)
    names = ["normal_a"] + C.case_names() + ["normal_b"]
    g = _batch(pkg, ctx, [cases[n] for n in names], tune)
    assert (g["status"] == 0).all(), g["status"]
    failures = []
    for i, n in enumerate(names):
        nk = cases[n]["n_kf"]
        T, inl = schedule_ref[n]
        got_T, got_inl = g["T"][i][:nk], g["inl"][g["lm_off"][i]:g["lm_off"][i + 1]]
        print("TOPO sched resident=%d waves=%-2d %-24s pose diff %.3e  flags differing %d of %d (%d flagged out)" % (resident, waves, n, np.abs(got_T - T).max(), int((got_inl != inl).sum()), len(inl), int((inl == 0).sum())))
        if not np.allclose(got_T, T, rtol=1e-4, atol=1e-6):
            failures.append((n, "poses", float(np.abs(got_T - T).max())))
        if not np.array_equal(got_inl, inl):
            failures.append((n, "flags", int((got_inl != inl).sum())))
        if n in ("zero_edges", "all_outliers_in") and not (_same_bits(got_T, g["T0"][i][:nk]) and np.array_equal(got_inl, g["inl0"][g["lm_off"][i]:g["lm_off"][i + 1]])):
            failures.append((n, "a window without an active edge was changed"))
    assert not failures, failures
    alone = _batch(pkg, ctx, [cases["normal_a"], cases["normal_b"]], tune)
    assert (alone["status"] == 0).all()
    for i, j in ((0, 0), (len(names) - 1, 1)):
        assert _same_bits(g["T"][i], alone["T"][j])
        assert np.array_equal(g["inl"][g["lm_off"][i]:g["lm_off"][i + 1]], alone["inl"][alone["lm_off"][j]:alone["lm_off"][j + 1]])
    assert not np.array_equal(g["T"][0], g["T0"][0])                                                  # the schedule moved the poses
