"""GPU: full_ba_kernel (vslam_full_ba_dev) over its input space -- held keyframes anywhere, the observation mask (holes in a landmark's range, a
landmark and a keyframe switched off entirely, observations behind the camera among the masked ones), the edge mask, edge weights per axis, edges
stored the other way round, in-place output -- against the numpy yardstick of tests/full_ba_ref.py.  tests/test_gpu_full_ba.py covers the sizes; the
cases are tests/full_ba_cases.py input_cases(), and tests/test_full_ba_ref.py guards every one of them and every bound asserted here."""
import numpy as np
import pytest

import full_ba_cases as Cs
import full_ba_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("T", "xyz", "obs_chi2", "stats")


def run(vo, problems, store=-1, **params):
    """the problems as one batch through VO.full_ba; camera and Huber width are the first problem's (one camera per call)"""
    b = Cs.pack(problems)
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


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


@pytest.mark.parametrize("store", [1, 0])
def test_evaluation_only(vo, store):
    """max_iters = 0 on one batch: chi2_init and the chi2 of EVERY observation against numpy at rtol 1e-9, the masked observations and edges left out
    of chi2_init, the observations behind the camera counted among those the mask left on only, poses and points copied"""
    cases = Cs.input_cases()
    names = ["obs_mask", "edge_weights", "edge_reversed", "edge_mask"]
    problems = [cases[n] for n in names]
    out = run(vo, problems, store, max_iters=0)
    for name, p, (T, X, chi2, st) in zip(names, problems, split(out, problems)):
        want = R.obs_chi2(p["T"], p["X"], p)
        act, dropped = R.input_active(p)
        print("%s: chi2_init %.9e (numpy %.9e), %d observations dropped, %d keyframes free" % (name, st["chi2_init"], R.cost(p["T"], p["X"], p), st["n_obs_dropped"], st["n_free"]))
        assert want.min() > 1e-8
        assert np.array_equal(T, p["T"]) and np.array_equal(X, p["X"])
        assert np.allclose(chi2, want, rtol=1e-9, atol=0)
        assert np.isclose(st["chi2_init"], R.cost(p["T"], p["X"], p), rtol=1e-9, atol=0) and st["chi2_final"] == st["chi2_init"]
        assert (st["lm_iters"], st["pcg_iters"], st["n_free"], st["n_obs_dropped"]) == (0, 0, int((~R.held_keyframes(p)).sum()), dropped)
        assert st["status"] == (R.FBA_DROPPED if dropped else 0)
        if name == "obs_mask":   # what the mask or the camera test left out is not in chi2_init, though it is in obs_chi2
            assert dropped > 0 and not np.isclose(st["chi2_init"], want.sum(), rtol=1e-3) and np.isclose(st["chi2_init"], want[act].sum(), rtol=1e-9, atol=0)
        if name == "edge_mask":
            assert not np.isclose(st["chi2_init"], R.cost(p["T"], p["X"], Cs.without(p, edge_active=None)), rtol=1e-3)
        if name in ("edge_weights", "edge_reversed"):   # (the edges are a visible part of the cost)
            assert R._edge_cost(p["T"], p) > 1e-3 * st["chi2_init"]


@pytest.mark.parametrize("store", [1, 0])
@pytest.mark.parametrize("name", Cs.INPUT_NAMES)
def test_parity(vo, name, store):
    """the bounds of tests/test_gpu_full_ba.py: chi2 values against numpy at the device's state at rtol 1e-9, poses and points within rtol 1e-4 / atol
    1e-6 of the yardstick's converged state, the exact gradient at most 1e-6 of the initial one, the cost fallen; what the case holds stays exactly
    where it was, and the counts are the yardstick's"""
    p, ref = Cs.input_reference(name)
    T, X, chi2, st = split(run(vo, [p], store), [p])[0]
    cost, gT, gX = R.cost_and_gradient(T, X, p)
    gn = float(np.sqrt((gT * gT).sum() + (gX * gX).sum()))
    g0 = Cs.gradient_norm(p, p["T"], p["X"])
    print("%s store %d: chi2 %.9e -> %.9e (numpy at the device's state %.9e, yardstick %.9e), gradient %.2e of initial, max |dT| %.2e, max |dX| %.2e, %d LM / %d PCG iterations, status %d"
          % (name, store, st["chi2_init"], st["chi2_final"], cost, ref["chi2_final"], gn / g0, np.abs(T - ref["T"]).max(), np.abs(X - ref["X"]).max(), st["lm_iters"],
             st["pcg_iters"], st["status"]))
    assert np.isclose(st["chi2_init"], ref["chi2_init"], rtol=1e-9, atol=0)
    assert np.isclose(st["chi2_final"], cost, rtol=1e-9, atol=0)
    assert np.allclose(chi2, R.obs_chi2(T, X, p), rtol=1e-9, atol=1e-24)
    assert np.allclose(T, ref["T"], rtol=1e-4, atol=1e-6)
    assert np.allclose(X, ref["X"], rtol=1e-4, atol=1e-6)
    assert gn <= 1e-6 * g0
    assert st["chi2_final"] < st["chi2_init"]
    assert 0 < st["lm_iters"] < R.DEFAULTS["max_iters"]
    hold, seen = R.held_keyframes(p), Cs.seen_landmarks(p)
    assert np.array_equal(T[hold], p["T"][hold]) and np.array_equal(X[~seen], p["X"][~seen])
    assert st["n_free"] == ref["n_free"] == int((~hold).sum())
    assert st["n_obs_dropped"] == R.input_active(p)[1] == ref["n_obs_dropped"]
    assert st["status"] == ref["status"] == (R.FBA_DROPPED if name == "obs_mask" else 0)
    if name == "obs_mask":   # the keyframe and the landmark whose observations are all off, and the landmark behind the camera
        assert hold[Cs.OBS_MASK["kf_off"]] and not seen[Cs.OBS_MASK["lm_off"]] and not seen[Cs.OBS_MASK["lm_behind"]] and st["n_free"] == 10
        assert 0 < st["n_obs_dropped"] < (p["lm"] == Cs.OBS_MASK["lm_behind"]).sum()


def _masked(p, held_kfs, edge_active):
    """p with held keyframes, an edge mask, and an observation mask that switches off every ninth observation that is not a landmark's first"""
    first = np.concatenate([[True], p["lm"][1:] != p["lm"][:-1]])
    on = ~((np.arange(len(p["kf"])) % 9 == 4) & ~first)
    return dict(p, fixed=Cs.held(len(p["T"]), held_kfs), edge_active=np.asarray(edge_active, np.uint8), obs_active=on.astype(np.uint8))


def _batches():
    """three problems of different sizes: `fixed`, an edge mask and an observation mask on the middle one only, and on all but the first"""
    plain2, plain65 = Cs.parity_cases()["arc_2_64"], Cs.parity_cases()["arc_65_65"]
    mid = _masked(Cs.parity_cases()["ring_5"], [0, 20], [1, 0, 1, 0, 1])
    last = _masked(Cs.ring(N=24, M=80, L=2), [3], [0, 1])
    return [plain2, mid, plain65], [plain2, mid, last]


@pytest.mark.parametrize("store", [1, 0])
def test_masks_and_held_keyframes_in_a_batch(vo, store):
    """the same call twice gives the same bytes, and every problem is bit for bit its output alone, where its own call passes NULL for what the batch
    had to fill in for it (keyframe 0 held, everything active)"""
    for problems in _batches():
        assert sum(p["fixed"] is None for p in problems) in (1, 2) and len({len(p["T"]) for p in problems}) == 3
        out = run(vo, problems, store)
        assert same_bytes(out, run(vo, problems, store))
        assert (out["stats"]["status"] == 0).all() and (out["stats"]["lm_iters"] > 0).all() and (out["stats"]["chi2_final"] < out["stats"]["chi2_init"]).all()
        for k, (p, part) in enumerate(zip(problems, split(out, problems))):
            alone = split(run(vo, [p], store), [p])[0]
            for a, b in zip(part, alone):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (store, k)
            hold = R.held_keyframes(p)
            assert np.array_equal(part[0][hold], p["T"][hold]) and part[3]["n_free"] == int((~hold).sum())


@pytest.mark.parametrize("store", [1, 0])
def test_in_place(vo, pkg, store):
    """vslam_full_ba_dev with d_T_out = d_T and d_xyz_out = d_xyz: the bytes of the call with outputs of its own, on three problems of which one is
    masked"""
    import ctypes as C
    import torch
    problems = _batches()[0]
    b = Cs.pack(problems)
    want = run(vo, problems, store)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p0 = problems[0]
    for in_place in (False, True):
        t = {k: up(b[k]) for k in ("kf_off", "lm_off", "obs_off", "edge_off", "T", "X", "kf", "lm", "uv", "disp", "ei", "ej", "Z", "w", "fixed", "obs_active", "edge_active")}
        t["chi2"] = torch.zeros(len(b["kf"]), dtype=torch.float64, device=dev)
        t["stats"] = torch.zeros(3 * pkg.FULL_BA_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        t["T_out"] = t["T"] if in_place else torch.zeros_like(t["T"])
        t["X_out"] = t["X"] if in_place else torch.zeros_like(t["X"])
        ptr = lambda k: t[k].data_ptr()
        ba = pkg.FullBABatch(n_problems=3, total_kfs=len(b["T"]), total_lms=len(b["X"]), total_obs=len(b["kf"]), total_edges=len(b["ei"]), d_kf_off=ptr("kf_off"),
                             d_lm_off=ptr("lm_off"), d_obs_off=ptr("obs_off"), d_edge_off=ptr("edge_off"), d_T=ptr("T"), d_fixed=ptr("fixed"), d_xyz=ptr("X"),
                             d_obs_kf=ptr("kf"), d_obs_lm=ptr("lm"), d_obs_uv=ptr("uv"), d_obs_disp=ptr("disp"), d_obs_active=ptr("obs_active"), d_obs_chi2=ptr("chi2"),
                             d_edge_i=ptr("ei"), d_edge_j=ptr("ej"), d_edge_Z=ptr("Z"), d_edge_w=ptr("w"), d_edge_active=ptr("edge_active"),
                             K4=(C.c_double * 4)(*p0["K4"]), bf=float(p0["bf"]), huber_delta=float(p0["huber"]))
        torch.cuda.synchronize()
        vo.set_tuning(fba_store=store)
        try:
            vo.full_ba_dev(ba, None, ptr("T_out"), ptr("X_out"), ptr("stats"))
            vo.sync()
        finally:
            vo.set_tuning(fba_store=-1)
        got = dict(T=t["T_out"].cpu().numpy(), xyz=t["X_out"].cpu().numpy(), obs_chi2=t["chi2"].cpu().numpy(), stats=t["stats"].cpu().numpy().view(pkg.FULL_BA_STATS_DTYPE))
        assert (ptr("T_out") == ptr("T") and ptr("X_out") == ptr("X")) == in_place
        assert same_bytes(got, want), in_place
    assert (want["stats"]["status"] == 0).all() and not np.array_equal(want["T"], b["T"]) and not np.array_equal(want["xyz"], b["X"])
