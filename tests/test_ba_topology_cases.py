"""CPU guards of the degenerate-graph BA cases (tests/ba_topology_cases.py), so that tests/test_gpu_ba_topology.py tests neither nothing nor chaos:
A the structure each name claims, B the oracle's trajectory is finite and significant for at least 3 iterations, C no chi2 that decides a landmark
flag sits within 1e-6 relative of its threshold (the GPU flags are then compared for equality), D recompute_chi2 reproduces the oracle's per-edge
chi2 and has teeth, E the oracle hands an edgeless keyframe's pose back bit for bit."""
import numpy as np
import pytest

import ba_topology_cases as C

NAMES = C.case_names()
HOST = [n for n in NAMES if n not in C.HOST_ONLY_SKIP]
TIE = 1e-6


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def runs(oracle, cases):
    """oracle.local_ba(iters = 8, both updates) and oracle.pose_only_window(iters = 8) per case, computed once"""
    out = {}
    for n in HOST:
        c = cases[n]
        out[n] = (oracle.local_ba(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], iters=8, update_poses=True, update_lms=True),
                  oracle.pose_only_window(c["T0"], c["xyz"], c["kf_idx"], c["lm_idx"], c["uv"], iters=8))
    return out


def _components(c):
    """connected components of the keyframe graph (keyframes joined by a shared landmark), as a sorted list of sorted lists"""
    parent = list(range(c["n_kf"]))
    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    first = {}
    for k, l in zip(c["kf_idx"].tolist(), c["lm_idx"].tolist()):
        if l in first:
            parent[find(k)] = find(first[l])
        else:
            first[l] = k
    groups = {}
    for k in range(c["n_kf"]):
        groups.setdefault(find(k), []).append(k)
    return sorted(groups.values())


def _shape(c):
    per_kf = np.bincount(c["kf_idx"], minlength=c["n_kf"])
    obs = np.bincount(c["lm_idx"], minlength=len(c["xyz"]))
    return per_kf, obs


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("name", list(C.SEEDS))
def test_case_is_a_valid_window(cases, name):
    c = cases[name]
    n_lm, ne = len(c["xyz"]), len(c["kf_idx"])
    assert c["T0"].shape == (c["n_kf"], 7) and c["xyz"].dtype == np.float32 and c["uv"].shape == (ne, 2) and 1 <= c["n_kf"] <= 12 and 1 <= n_lm <= 300
    assert len(c["lm_idx"]) == ne and c["kf_idx"].dtype == np.int32 and c["lm_idx"].dtype == np.int32
    assert np.isfinite(c["T0"]).all() and np.isfinite(c["xyz"]).all() and np.isfinite(c["uv"]).all()
    if ne:
        assert c["kf_idx"].min() >= 0 and c["kf_idx"].max() < c["n_kf"] and c["lm_idx"].min() >= 0 and c["lm_idx"].max() < n_lm
        assert (np.diff(c["lm_idx"]) >= 0).all()                                                       # sorted by landmark: the batched entry's contract
        assert len(set(zip(c["kf_idx"].tolist(), c["lm_idx"].tolist()))) == ne                         # no duplicate edge
    if name not in ("unobserved_interleaved", "zero_edges"):
        assert (_shape(c)[1] >= 1).all(), "a landmark without an edge was not re-numbered away"


@pytest.mark.parametrize("name,k", list(C.EMPTY_KF.items()))
def test_empty_keyframe_cases(cases, name, k):
    per_kf, obs = _shape(cases[name])
    assert per_kf[k] == 0 and (np.delete(per_kf, k) >= 20).all()
    comps = _components(cases[name])
    assert [k] in comps
    if name == "kf_mid_empty":
        assert obs.max() >= 2 and len(comps) >= 2


@pytest.mark.parametrize("name,n", [("kf_one_edge", 1), ("kf_two_edges", 2)])
def test_few_edge_keyframe_cases(cases, name, n):
    per_kf, _ = _shape(cases[name])
    assert per_kf[3] == n and (np.delete(per_kf, 3) >= 20).all()


def test_disconnected_case(cases):
    c = cases["disconnected"]
    assert _components(c) == [[0, 1, 2], [3, 4, 5]]
    side = c["kf_idx"] < 3
    for l in np.unique(c["lm_idx"]):
        assert len(set(side[c["lm_idx"] == l].tolist())) == 1
    assert (_shape(c)[0] >= 10).all() and (_shape(c)[1] >= 2).any()


def test_observation_histograms(cases):
    per_kf, obs = _shape(cases["all_singles"])
    assert (obs == 1).all() and len(obs) == 150 and cases["all_singles"]["n_kf"] == 6 and (per_kf > 0).all()
    assert len(_components(cases["all_singles"])) == 6                                                # nothing couples two keyframes
    c = cases["all_see_all"]
    per_kf, obs = _shape(c)
    assert c["n_kf"] == 12 and len(obs) == 40 and (obs == 12).all() and (per_kf == 40).all() and len(c["kf_idx"]) == 480
    for n in (63, 64, 65, 129):
        _, obs = _shape(cases["rows_%d" % n])
        assert len(obs) == n and obs.min() >= 2 and obs.max() <= 4
    for n in (255, 256, 257):
        c = cases["edges_%d" % n]
        assert len(c["kf_idx"]) == n and _shape(c)[1].min() >= 1
    c = cases["unobserved_interleaved"]
    _, obs = _shape(c)
    un = np.flatnonzero(obs == 0)
    assert len(obs) == 150 and np.array_equal(un, np.arange(2, 150, 5)) and un[-1] < 149 and (obs[un + 1] > 0).all()
    c = cases["one_edge"]
    assert c["n_kf"] == 1 and len(c["xyz"]) == 1 and len(c["kf_idx"]) == 1
    c = cases["zero_edges"]
    assert c["n_kf"] == 6 and len(c["xyz"]) == 20 and len(c["kf_idx"]) == 0
    c = cases["all_outliers_in"]
    assert c["inl0"].dtype == np.uint8 and not c["inl0"].any() and len(c["inl0"]) == len(c["xyz"]) and len(c["kf_idx"]) > 300


def test_behind_camera_case(cases):
    c = cases["behind_camera"]
    l, k = c["moved"]
    e = np.flatnonzero(c["lm_idx"] == l)
    assert len(e) >= 2 and c["kf_idx"][e[0]] == k
    z = C._camera_points(c["T0"], c["xyz"], c["kf_idx"][e], c["lm_idx"][e])[:, 2]
    assert abs(z[0] + 5.0) < 1e-4 and (z < 0).all()
    others = np.flatnonzero(c["lm_idx"] != l)
    assert (C._camera_points(c["T0"], c["xyz"], c["kf_idx"][others], c["lm_idx"][others])[:, 2] > 1.0).all()


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("name", HOST)
def test_oracle_trajectory_is_finite_and_significant(cases, runs, name):
    (T, xyz, chi2, st), (Tp, chi2p, stp) = runs[name]
    for a in (T, xyz, chi2, Tp, chi2p, st["chi2_iter"], st["lambda_iter"], stp["chi2_iter"], stp["lambda_iter"]):
        assert np.isfinite(a).all()
    if name in C.NO_TRAJECTORY:
        return
    assert C.significant_prefix(st) >= 3, (st["chi2_init"], st["chi2_iter"])
    assert C.significant_prefix(stp) >= 3, (stp["chi2_init"], stp["chi2_iter"])
    assert st["trials_iter"][:3] == [1, 1, 1] and stp["trials_iter"][:3] == [1, 1, 1]
    # and no iteration starts below the f64 evaluation floor of the cost: the GPU tests compare the whole record of these windows
    floor = C.chi2_floor(cases[name]["uv"])
    for s in (st, stp):
        assert min([s["chi2_init"]] + s["chi2_iter"][:-1]) > floor


# ------------------------------------------------------------------------------------------------ C
def _no_tie(chi2, th, flag_lm, n_lm):
    if len(chi2) == 0:
        return
    # the threshold itself: the count that decides a doubling must not hinge on a tie either
    t = C.CHI2_TH0
    while True:
        assert (np.abs(chi2 - t) > TIE * t).all(), (t, chi2[np.abs(chi2 - t) <= TIE * t])
        if t >= th:
            break
        t *= 2
    d = chi2[C.deciding_edges(flag_lm, n_lm)]
    assert (np.abs(d - th) > TIE * th).all()


@pytest.mark.parametrize("name", list(C.SEEDS))
def test_no_flag_is_decided_by_a_tie(oracle, cases, runs, name):
    c = cases[name]
    trace = []
    C.oracle_schedule(oracle, c, trace)
    assert len(trace) == 4
    for chi2, th, flag_lm in trace:
        _no_tie(chi2, th, flag_lm, len(c["xyz"]))
    if name in runs:
        for chi2 in (runs[name][0][2], runs[name][1][1]):
            th, _, _, _ = oracle.chi2_classify(chi2, c["lm_idx"], np.ones(len(c["xyz"]), np.uint8))
            _no_tie(chi2, th, c["lm_idx"], len(c["xyz"]))


def test_schedule_leaves_degenerate_windows_alone(oracle, cases):
    for name in ("zero_edges", "all_outliers_in"):
        c = cases[name]
        T, inl = C.oracle_schedule(oracle, c)
        assert np.array_equal(T, c["T0"]) and np.array_equal(inl, c.get("inl0", np.ones(len(c["xyz"]), np.uint8)))


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("name", [n for n in HOST if n != "zero_edges"])
def test_recompute_chi2_reproduces_the_oracle(oracle, cases, runs, name):
    """pose-only: the oracle's state is its output (poses f64, landmarks the f32 input), so its per-edge chi2 is reproduced to 1e-9 relative (plus
    1e-12 px^2, the floor of two f64 evaluations of a residual that the one-edge case drives to zero).  optimize_map: the oracle evaluates at f64
    landmark positions and hands out their f32 roundings, so the per-edge allowance for that storage applies, derived in f32_storage_allowance.  Both at
    the longest prefix of the run that ends in an accepted step: the chi2 record is that of the last trial, the state that of the last accepted one."""
    c = cases[name]
    kf, lm, uv = c["kf_idx"], c["lm_idx"], c["uv"]
    (_, _, _, st), (_, _, stp) = runs[name]
    n = C.last_accepted_iteration(stp)
    assert n >= 1
    T, chi2, st2 = oracle.pose_only_window(c["T0"], c["xyz"], kf, lm, uv, iters=n)
    assert st2["chi2_iter"] == stp["chi2_iter"][:n]
    mine, total = C.recompute_chi2(T, c["xyz"], kf, lm, uv)
    assert np.allclose(mine, chi2, rtol=1e-9, atol=1e-12), np.abs(mine - chi2).max()
    assert np.isclose(total, st2["chi2_final"], rtol=1e-9, atol=1e-12)
    first, _ = C.recompute_chi2(c["T0"], c["xyz"], kf, lm, uv)
    assert np.isclose(C.huber_sum(first), stp["chi2_init"], rtol=1e-9)
    # teeth: one output pose translated by 1e-6 m moves some edge by more than the tolerance
    T2 = T.copy(); T2[c["n_kf"] - 1 if name not in C.EMPTY_KF else (C.EMPTY_KF[name] + 1) % c["n_kf"], 4] += 1e-6
    moved, _ = C.recompute_chi2(T2, c["xyz"], kf, lm, uv)
    assert (np.abs(moved - chi2) > 1e-9 * chi2 + 1e-12).any()
    # optimize_map
    n = C.last_accepted_iteration(st)
    assert n >= 1
    T, xyz, chi2, st2 = oracle.local_ba(c["T0"], c["xyz"], kf, lm, uv, iters=n, update_poses=True, update_lms=True)
    mine, _ = C.recompute_chi2(T, xyz, kf, lm, uv)
    allow = C.f32_storage_allowance(T, xyz, kf, lm, uv)
    assert (np.abs(mine - chi2) <= allow).all(), (np.abs(mine - chi2).max(), allow.max())


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("name,k", list(C.EMPTY_KF.items()))
def test_oracle_returns_the_edgeless_pose_bit_for_bit(cases, runs, name, k):
    (T, _, _, _), (Tp, _, _) = runs[name]
    T0 = cases[name]["T0"]
    assert T[k].tobytes() == T0[k].tobytes() and Tp[k].tobytes() == T0[k].tobytes()
    assert not np.array_equal(np.delete(T, k, 0), np.delete(T0, k, 0))
