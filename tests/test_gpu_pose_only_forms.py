"""pose_only_wave_kernel runs a window on 12 waves (one keyframe per wave) or on fewer, each wave then taking a list of keyframes dealt by active
edge count.  A keyframe's sums do not depend on the wave that forms them, so every form must give the SAME BITS: the device schedule is run on the
same windows with pose_only_waves = 12 and with the narrow form, and every output is compared for equality (NaN equal to NaN), not closeness.

vslam_ba_batch_dev does not hand out the final chi2 threshold of a window (its chi2_thr is internal to the launch); the landmark flags, which are
`chi2 <= threshold` of each landmark's last edge, and the per-edge chi2 are compared instead."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KF_MAX = 12
NARROW_WAVES = (4,)   # the narrow instantiations of the library (kPoseOnlyNarrowWaves in csrc/vslam_internal.h)
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
STATS = np.dtype([("iterations", "<i4"), ("total_trials", "<i4"), ("chi2_init", "<f8"), ("chi2_final", "<f8"), ("lambda_final", "<f8"),
                  ("chi2_iter", "<f8", 32), ("lambda_iter", "<f8", 32), ("trials_iter", "<i4", 32)])


def _one_keyframe_heavy(synth, seed, k_star=4, keep=0.05):
    """the landmarks that keyframe k_star sees, with their edge in k_star and one in twenty of their other edges"""
    w = synth.ba_window_fast(n_kf=10, n_lm=1300, seed=seed)
    rng = np.random.default_rng(seed)
    seen = np.zeros(len(w["xyz"]), bool)
    seen[w["lm_idx"][w["kf_idx"] == k_star]] = True
    e = seen[w["lm_idx"]] & ((w["kf_idx"] == k_star) | (rng.random(len(w["kf_idx"])) < keep))
    new_id = np.cumsum(seen) - 1
    return dict(T0=w["T0"], xyz=w["xyz"][seen], kf_idx=w["kf_idx"][e], lm_idx=new_id[w["lm_idx"][e]].astype(np.int32), uv=w["uv"][e])


def _windows(synth):
    """(window, its keyframe count, landmarks handed in as outliers).  Keyframe counts below, at and between the multiples of the narrow forms, the
    maximum, and 1; per-window counts below the stride of 12"""
    wins = []
    for i, (nk, nl) in enumerate(((12, 400), (10, 700), (7, 300), (5, 250))):
        wins.append([synth.ba_window_fast(n_kf=nk, n_lm=nl, seed=700 + i), nk, None])
    wins.append([synth.ba_window_fast(n_kf=2, n_lm=200, seed=710, min_obs=2, max_obs=2), 2, None])
    wins.append([synth.ba_window_fast(n_kf=1, n_lm=200, seed=711, min_obs=1, max_obs=1), 1, None])
    wins.append([_one_keyframe_heavy(synth, 712), 10, None])
    # gross outliers and a bad start: trials get rejected, and fewer than half of the edges pass the first classification threshold
    wins.append([synth.ba_window_fast(n_kf=10, n_lm=300, seed=713, outlier_frac=0.6, pose_sigma=0.08), 10, None])
    # window 0: every landmark that the last keyframe sees is handed in as an outlier, so that keyframe has no active edge at all
    w0 = wins[0][0]
    off = np.zeros(len(w0["xyz"]), bool)
    off[w0["lm_idx"][w0["kf_idx"] == 11]] = True
    assert off.any() and not off.all()
    wins[0][2] = off
    return wins


def _run(pkg, ctx, wins, stride, waves, per_window_nkf=True, want_stats=True):
    import torch
    d = "cuda"
    n = len(wins)
    lm_off = np.cumsum([0] + [len(w["xyz"]) for w, _, _ in wins]).astype(np.int32)
    e_off = np.cumsum([0] + [len(w["kf_idx"]) for w, _, _ in wins]).astype(np.int32)
    T0 = np.tile(IDENT, (n, stride, 1))
    inl0 = np.ones(int(lm_off[-1]), np.uint8)
    for i, (w, nk, off) in enumerate(wins):
        T0[i, :nk] = w["T0"]
        if off is not None:
            inl0[lm_off[i]:lm_off[i + 1]][off] = 0
    T = torch.from_numpy(T0).to(d)
    xyz = torch.from_numpy(np.concatenate([w["xyz"] for w, _, _ in wins])).to(d)
    kf = torch.from_numpy(np.concatenate([w["kf_idx"] for w, _, _ in wins])).to(d)
    lm = torch.from_numpy(np.concatenate([w["lm_idx"] for w, _, _ in wins])).to(d)
    uv = torch.from_numpy(np.concatenate([w["uv"] for w, _, _ in wins])).to(d)
    inl = torch.from_numpy(inl0).to(d)
    chi = torch.zeros(int(e_off[-1]), dtype=torch.float64, device=d)
    st = torch.zeros(n * STATS.itemsize, dtype=torch.uint8, device=d)
    nkf = torch.from_numpy(np.array([nk for _, nk, _ in wins], np.int32)).to(d)
    t_lm, t_e = torch.from_numpy(lm_off).to(d), torch.from_numpy(e_off).to(d)
    bb = pkg.BaBatch()
    bb.n_windows = n; bb.n_kf = stride
    bb.d_lm_off = t_lm.data_ptr(); bb.d_edge_off = t_e.data_ptr(); bb.d_T_c_w = T.data_ptr(); bb.d_xyz = xyz.data_ptr()
    bb.d_reliable = None; bb.d_lm_inlier = inl.data_ptr(); bb.d_kf_idx = kf.data_ptr(); bb.d_lm_idx = lm.data_ptr(); bb.d_uv = uv.data_ptr()
    bb.d_chi2 = chi.data_ptr(); bb.d_stats = st.data_ptr() if want_stats else None; bb.total_lm = int(lm_off[-1]); bb.total_edge = int(e_off[-1])
    bb.d_n_kf = nkf.data_ptr() if per_window_nkf else None
    ctx.set_tuning(pose_only_waves=waves)
    torch.cuda.synchronize()
    ctx.ba_batch_dev(bb, schedule=1)
    ctx.sync()
    ctx.set_tuning(pose_only_waves=-1)
    assert (ctx.ba_status(n) == 0).all()
    return dict(T=T.cpu().numpy(), inl=inl.cpu().numpy(), chi2=chi.cpu().numpy(), stats=st.cpu().numpy().view(STATS), T0=T0, inl0=inl0, e_off=e_off)


def _same_bits(a, b):
    assert np.array_equal(a["T"], b["T"], equal_nan=True), np.nanmax(np.abs(a["T"] - b["T"]))
    assert np.array_equal(a["inl"], b["inl"])
    assert np.array_equal(a["chi2"], b["chi2"], equal_nan=True), np.nanmax(np.abs(a["chi2"] - b["chi2"]))
    for f in STATS.names:
        x, y = a["stats"][f], b["stats"][f]
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y), f


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.VO(device=0, max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wins(synth):
    return _windows(synth)


@pytest.fixture(scope="module")
def wide(pkg, ctx, wins):
    """the windows on one keyframe per wave, computed once"""
    return _run(pkg, ctx, wins, KF_MAX, KF_MAX)


def test_the_windows_are_the_hard_ones(wins, wide):
    """the inputs do what they are there for (checked on the 12-wave form)"""
    ne = np.diff(wide["e_off"])
    for W in NARROW_WAVES:
        assert (ne % (64 * W) != 0).any()
    heavy = wins[6][0]["kf_idx"]
    assert (heavy == 4).mean() > 0.75
    st = wide["stats"]
    assert (st["total_trials"] > st["iterations"]).any(), "no window rejected a trial"
    assert not np.array_equal(wide["T"][:, 0], wide["T0"][:, 0])   # the schedule moved the poses
    assert not np.array_equal(wide["inl"], wide["inl0"])
    # the last keyframe of window 0 had nothing to go by in the pose-only pass, its landmarks stay out
    off = wins[0][2]
    assert (wide["inl"][:len(off)][off] == 0).all() and np.isfinite(wide["T"][0]).all()


@pytest.mark.parametrize("W", NARROW_WAVES)
def test_narrow_form_gives_the_bits_of_one_keyframe_per_wave(pkg, ctx, wins, wide, W):
    _same_bits(wide, _run(pkg, ctx, wins, KF_MAX, W))


@pytest.mark.parametrize("W", NARROW_WAVES)
def test_narrow_form_without_per_window_keyframe_counts(pkg, ctx, synth, W):
    """n_kf is the stride and the count of every window (no d_n_kf): 10 keyframes, not a multiple of every narrow form"""
    ws = [[synth.ba_window_fast(n_kf=10, n_lm=200 + 150 * i, seed=730 + i), 10, None] for i in range(3)]
    a = _run(pkg, ctx, ws, 10, KF_MAX, per_window_nkf=False)
    _same_bits(a, _run(pkg, ctx, ws, 10, W, per_window_nkf=False))


def test_automatic_form_on_a_launch_larger_than_the_device(pkg, ctx, synth):
    """about 300 tiny windows: more windows than CUs, so pose_only_waves = 0 takes whatever the launcher picks for large launches"""
    ws = [[synth.ba_window_fast(n_kf=2, n_lm=30, seed=800 + i, min_obs=2, max_obs=2), 2, None] for i in range(300)]
    a = _run(pkg, ctx, ws, 2, KF_MAX)
    _same_bits(a, _run(pkg, ctx, ws, 2, 0))


@pytest.mark.parametrize("W", NARROW_WAVES[:1])
def test_narrow_form_on_built_windows_matches_oracle(oracle, synth, W):
    """tests/test_gpu_windows.py::test_ba_schedule_on_built_windows_matches_oracle with the pose-only pass forced to the narrow form: the oracle's
    composite schedule per window, optimize_pose_only last, that test's tolerance"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 12, 10
    pipe = KeyframePipeline(B, anms_num=500, n_kf=n_kf, unique_frames=B, seed=6, ba_windows="tracks")
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        built = pipe.download()
        pipe.vo.set_tuning(pose_only_waves=W)
        pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        done = pipe.download()
        assert (pipe.vo.ba_status(B) == 0).all() and built["ba_build_status"][0] == 0
        lm_off, e_off = built["ba_lm_off"], built["ba_e_off"]
        for b in (0, 1, 4, 9, 11):
            nk = int(built["ba_nkf"][b])
            kf, lm, uv = (built[k][e_off[b]:e_off[b + 1]] for k in ("ba_kf", "ba_lm", "ba_uv"))
            xyz = built["ba_xyz"][lm_off[b]:lm_off[b + 1]]; rel = built["ba_rel"][lm_off[b]:lm_off[b + 1]].astype(bool)
            T = built["ba_T"][b][:nk].copy(); inl = np.ones(len(xyz), np.uint8)
            for iters, upd in ((5, False), (5, False), (10, True)):
                act = (inl.astype(bool) & rel)[lm]
                T2, _, chi2, _ = oracle.local_ba(T, xyz, kf[act], lm[act], uv[act], iters=iters)
                _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
                if upd:
                    T = T2
            act = inl.astype(bool)[lm]
            T2, chi2, _ = oracle.pose_only_window(T, xyz, kf[act], lm[act], uv[act], iters=10)
            _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
            assert np.allclose(done["ba_T"][b][:nk], T2, rtol=1e-4, atol=1e-6), (b, np.abs(done["ba_T"][b][:nk] - T2).max())
            got = done["ba_inl"][lm_off[b]:lm_off[b + 1]]
            assert np.array_equal(got, inl), (b, int((got != inl).sum()))
    finally:
        pipe.close()
