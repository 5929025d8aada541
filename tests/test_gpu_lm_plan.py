"""What launch_lm_windows / launch_pnp decide per call -- which kernels take the windows, adaptive or plain schedule, the pose-only form, the width of
ba_resident_kernel, the launch count reported to the stage profiler -- and the last-launch record behind vslam_ba_status_dev,
vslam_ba_schedule_passes_dev and vslam_ba_deferred_dev, pinned through what a caller can observe: ba_deferred, ba_schedule_passes, profile_read,
ba_status, and the bits of the results where two choices promise the same bits.  The windows are the smallest that still take each path: three
windows of 4 keyframes and 100 landmarks, `sparse` with 1-2 observations per landmark (the default rule gives them to ba_resident_kernel) and
`dense` with 3-4 (above 2.2 per landmark: the default rule leaves them to lm_window_kernel)."""
import numpy as np
import pytest

from test_gpu_ba_chain import ANMS, seq8  # noqa: F401  (the 8 rendered frames of the chain tests)

pytestmark = pytest.mark.gpu

N_WIN, N_KF, N_LM = 3, 4, 100
OBS = {"sparse": (1, 2), "dense": (3, 4)}
TUNING_KEYS = ("ba_resident", "ba_adaptive", "ba_lanes", "pose_only_waves", "pose_only_window", "pnp_window")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.VO(device=0, max_batch=1)
    c.profile_enable(True)
    yield c
    c.close()


class _Batch:
    """three windows on the device; run() restores the inputs, sets the tuning, makes ONE vslam_ba_batch_dev call and returns what it left"""

    def __init__(self, pkg, synth, kind, bad_window=None):
        import torch
        self.torch = torch
        lo, hi = OBS[kind]
        ws = [synth.ba_window_fast(n_kf=N_KF, n_lm=N_LM, seed=900 + i, min_obs=lo, max_obs=hi) for i in range(N_WIN)]
        if bad_window is not None:   # a duplicate (keyframe, landmark) edge, next to its original: the kernels reject the window, its status word is not 0
            w = ws[bad_window]
            for k in ("kf_idx", "lm_idx", "uv"):
                w[k] = np.concatenate([w[k][:1], w[k]])
        self.obs_per_lm = [len(w["kf_idx"]) / len(w["xyz"]) for w in ws]
        lm_off = np.cumsum([0] + [len(w["xyz"]) for w in ws]).astype(np.int32)
        e_off = np.cumsum([0] + [len(w["kf_idx"]) for w in ws]).astype(np.int32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        self.T0 = t(np.stack([w["T0"] for w in ws]))
        self.T = self.T0.clone()
        self.inl = torch.ones(int(lm_off[-1]), dtype=torch.uint8, device="cuda")
        self.chi2 = torch.zeros(int(e_off[-1]), dtype=torch.float64, device="cuda")
        self.keep = [t(lm_off), t(e_off), t(np.concatenate([w["xyz"] for w in ws])), t(np.concatenate([w["kf_idx"] for w in ws])),
                     t(np.concatenate([w["lm_idx"] for w in ws])), t(np.concatenate([w["uv"] for w in ws]))]
        d_lo, d_eo, xyz, kf, lm, uv = self.keep
        b = pkg.BaBatch()
        b.n_windows = N_WIN; b.n_kf = N_KF; b.d_lm_off = d_lo.data_ptr(); b.d_edge_off = d_eo.data_ptr(); b.d_T_c_w = self.T.data_ptr(); b.d_xyz = xyz.data_ptr()
        b.d_reliable = None; b.d_lm_inlier = self.inl.data_ptr(); b.d_kf_idx = kf.data_ptr(); b.d_lm_idx = lm.data_ptr(); b.d_uv = uv.data_ptr()
        b.d_chi2 = self.chi2.data_ptr(); b.d_stats = None; b.total_lm = int(lm_off[-1]); b.total_edge = int(e_off[-1])
        self.b = b

    def run(self, ctx, schedule=1, mode=0, **tuning):
        self.T.copy_(self.T0); self.inl.fill_(1); self.chi2.zero_()
        self.torch.cuda.synchronize()   # (the copies run on torch's stream, the library on its own)
        ctx.set_tuning(**{k: tuning.get(k, -1) for k in TUNING_KEYS})
        ctx.profile_read()
        try:
            ctx.ba_batch_dev(self.b, schedule=schedule, mode=mode, iters=5, update_poses=1, update_lms=0)
            prof = ctx.profile_read()
        finally:
            ctx.set_tuning(**{k: -1 for k in TUNING_KEYS})
        return dict(prof=prof, status=ctx.ba_status(N_WIN), passes=ctx.ba_schedule_passes(N_WIN), deferred=ctx.ba_deferred(N_WIN),
                    T=self.T.cpu().numpy().view(np.uint64), inl=self.inl.cpu().numpy(), chi2=self.chi2.cpu().numpy().view(np.uint64))


@pytest.fixture(scope="module")
def batches(pkg, synth):
    return {kind: _Batch(pkg, synth, kind) for kind in OBS}


def test_the_windows_sit_on_both_sides_of_the_dense_rule(batches):
    assert all(r < 2.0 for r in batches["sparse"].obs_per_lm) and all(r > 3.0 for r in batches["dense"].obs_per_lm)


# ------------------------------------------------------------------ a. who took the windows
@pytest.mark.parametrize("kind", list(OBS))
def test_deferred_follows_ba_resident_and_the_dense_rule(ctx, batches, kind):
    bt = batches[kind]
    for resident, want in ((0, 1), (1, 0), (-1, 0 if kind == "sparse" else 1)):
        r = bt.run(ctx, ba_resident=resident)
        assert (r["status"] == 0).all()
        assert (r["deferred"] == want).all(), (kind, resident, r["deferred"])
    r = bt.run(ctx, schedule=0, mode=1)   # a single pose-only pass: ba_resident_kernel is not involved
    assert (r["status"] == 0).all() and (r["deferred"] == 1).all(), (kind, r["deferred"])


# ------------------------------------------------------------------ b. the passes executed, and the choices that promise the same bits
@pytest.mark.parametrize("kind", list(OBS))
def test_schedule_passes_and_bit_identical_forms(ctx, batches, kind):
    bt = batches[kind]
    assert (bt.run(ctx, ba_adaptive=0)["passes"] == 3).all()
    base = bt.run(ctx)
    assert (base["status"] == 0).all() and np.isin(base["passes"], (1, 2, 3)).all(), base["passes"]
    assert not np.array_equal(base["T"], bt.T0.cpu().numpy().view(np.uint64))   # the schedule moved the poses
    for key, values, same_bits in (("ba_lanes", (256, 512), True), ("pose_only_waves", (4, 12), True), ("pose_only_window", (0, 1), False)):
        for v in values:
            r = bt.run(ctx, **{key: v})
            assert (r["status"] == 0).all() and np.array_equal(r["passes"], base["passes"]), (kind, key, v, r["passes"], base["passes"])
            if same_bits:
                for k in ("T", "inl", "chi2"):
                    assert np.array_equal(r[k], base[k]), (kind, key, v, k)


# ------------------------------------------------------------------ c. the launch counts the stage profiler is told
@pytest.mark.parametrize("resident", [0, 1, -1])
def test_profiler_launch_counts_of_the_ba_calls(ctx, batches, resident):
    bt = batches["sparse"]
    r1 = 1 if resident != 0 else 0   # ba_resident_kernel is involved in a schedule or a mode-0 pass unless ba_resident = 0
    for call, want in ((dict(schedule=0, mode=0), 1 + r1), (dict(schedule=0, mode=1), 1), (dict(schedule=1), 2 + r1), (dict(schedule=1, ba_adaptive=0), 4 + r1)):
        prof = bt.run(ctx, ba_resident=resident, **call)["prof"]
        assert set(prof) == {"lm_window_kernel"} and prof["lm_window_kernel"][1:] == (want, 1), (resident, call, prof)


def _pose_call(ctx, synth, pnp_window):
    """vslam_pnp_motion_only_dev on two small problems; the profiler's families and the poses"""
    import torch
    B, cap = 2, 64
    xyz = np.zeros((B, cap, 3), np.float32); uv = np.zeros((B, cap, 2), np.float32); n = np.zeros(B, np.int32); T = np.zeros((B, 7))
    for b in range(B):
        p = synth.pnp_problem(M=50 + 10 * b, seed=3 + b)
        m = len(p["xyz"]); xyz[b, :m] = p["xyz"]; uv[b, :m] = p["uv"]; n[b] = m; T[b] = p["T0"]
    t = lambda a: torch.from_numpy(a).to("cuda")
    dx, du, dn, dT = t(xyz), t(uv), t(n), t(T)
    dinl = torch.zeros((B, cap), dtype=torch.uint8, device="cuda"); dni = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.set_tuning(pnp_window=pnp_window)
    ctx.profile_read()
    try:
        ctx.motion_estimation_dev(dx.data_ptr(), du.data_ptr(), dn.data_ptr(), cap, B, dT.data_ptr(), 10, dinl.data_ptr(), dni.data_ptr())
        prof = ctx.profile_read()
    finally:
        ctx.set_tuning(pnp_window=-1)
    return prof, dT.cpu().numpy(), dni.cpu().numpy()


def test_profiler_launch_counts_of_the_pose_calls(ctx, synth):
    prof, T_wave, n_wave = _pose_call(ctx, synth, -1)
    assert set(prof) == {"pnp_wave_kernel"} and prof["pnp_wave_kernel"][1:] == (1, 1), prof
    prof, T_win, n_win = _pose_call(ctx, synth, 1)
    assert set(prof) == {"lm_window_kernel<pnp>"} and prof["lm_window_kernel<pnp>"][1:] == (2, 1), prof
    assert (n_wave > 20).all() and np.array_equal(n_wave, n_win) and np.allclose(T_wave, T_win, rtol=1e-6, atol=1e-9)   # (both forms solved the problems)


# ------------------------------------------------------------------ d. after a chain: the caller's windows' status words, no per-launch diagnostics
def test_record_after_a_chain(pkg, seq8):  # noqa: F811
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    n = 8
    pipe = KeyframePipeline(n, anms_num=ANMS, n_kf=N_KF, unique_frames=8, seed=6, sequence=seq8, ba_windows="tracks", ba_chain=True, ba_chain_min_kf=1)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_ba()
        status = pipe.vo.ba_status(n)
        assert status.shape == (n,) and (status == 0).all() and pipe.ba_ran.cpu().numpy().all()
        for fetch in (pipe.vo.ba_schedule_passes, pipe.vo.ba_deferred):
            with pytest.raises(pkg.VslamError):
                fetch(n)
        assert (pipe.vo.ba_status(n) == 0).all()   # (a refused fetch changes nothing)
    finally:
        pipe.close()


# ------------------------------------------------------------------ e. the record is replaced whole by every launch that carves the scratch
def test_record_is_replaced_whole(ctx, pkg, synth):
    bt = _Batch(pkg, synth, "sparse", bad_window=1)
    first = bt.run(ctx)
    assert first["status"][1] != 0 and first["status"][0] == 0 and first["status"][2] == 0, first["status"]
    _pose_call(ctx, synth, 1)   # lm_window_kernel<pnp> on two problems carves the same scratch: the record now describes that launch
    assert (ctx.ba_status(2) == 0).all()
    again = bt.run(ctx)
    for k in ("status", "passes", "deferred"):
        assert np.array_equal(again[k], first[k]), (k, again[k], first[k])
    assert (again["deferred"] == 0).all()
