#!/usr/bin/env python3
"""micro-benchmark: batched cross-check matcher only (B items of N x N random descriptors), for kernel tuning.
--select P [P ...]: also time vslam_feature_matching_subset_dev on the same items with a random ascending P % of every item's query rows selected
(100: every row -- the unmasked call's output); a selection is compacted, so its cost follows its length"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import stereo_visual_slam_amd as pkg
ap = argparse.ArgumentParser(); ap.add_argument("--batch", type=int, default=256); ap.add_argument("--rows", type=int, default=1500)
ap.add_argument("--cap", type=int, default=4096); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--select", type=float, nargs="*", default=[], help="percent of the query rows in the subset call's selection")
a = ap.parse_args()
B, N, cap = a.batch, a.rows, a.cap
vo = pkg.VO(device=0, max_batch=B)
g = torch.Generator(device="cuda"); g.manual_seed(0)
q = torch.randint(0, 256, (B, cap, 32), dtype=torch.uint8, device="cuda", generator=g)
t = torch.randint(0, 256, (B, cap, 32), dtype=torch.uint8, device="cuda", generator=g)
n = torch.full((2 * B,), N, dtype=torch.int32, device="cuda")
gap = torch.ones(B, dtype=torch.float64, device="cuda")
out = torch.empty((B, cap, 16), dtype=torch.uint8, device="cuda"); nout = torch.zeros(B, dtype=torch.int32, device="cuda")
run = lambda: vo.feature_matching_dev(q.data_ptr(), cap * 32, n.data_ptr(), t.data_ptr(), cap * 32, n.data_ptr() + 4 * B, gap.data_ptr(), 1, B, cap,
                                      out.data_ptr(), cap, nout.data_ptr())
run(); vo.sync(); vo.profile_enable(True); vo.profile_read()
t0 = time.perf_counter()
for _ in range(a.reps): run()
vo.sync(); dt = (time.perf_counter() - t0) / a.reps
pr = vo.profile_read()
print("B=%d N=%d  %.3f ms/call  %.2f T pair-distances/s" % (B, N, dt * 1e3, B * N * N / dt / 1e12))
print({k: round(v[0] / a.reps, 4) for k, v in sorted(pr.items(), key=lambda kv: -kv[1][0])})
# issue floor of the Hamming table: four v_mfma_f32_32x32x64_f8f6f4 (FP4) per 32 x 32 block at 32.5 cycles each (tools/scratch/mfma_fp4_layout.hip), column
# tiles in whole workgroups of 512 columns, one matrix pipe per SIMD, nominal 2.4 GHz
simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
floor_ms = B * ((N + 31) // 32) * (16 * ((N + 511) // 512)) * 4 * 32.5 / (simds * 2.4e9) * 1e3
k_ms = pr.get("match_train_nearest_kernel", (0.0,))[0] / a.reps
if k_ms > 0:
    print("match_train_nearest_kernel %.4f ms = %.0f %% of its MFMA issue floor (%.4f ms, FP4 32x32x64)" % (k_ms, 100.0 * floor_ms / k_ms, floor_ms))
for pct in a.select:
    k = max(0, min(N, int(round(N * pct / 100.0))))
    rs = np.random.default_rng(1)
    sel = np.zeros((B, cap), np.int32)
    for b in range(B):
        sel[b, :k] = np.sort(rs.permutation(N)[:k])
    d_sel = torch.from_numpy(sel).cuda(); d_nsel = torch.full((B,), k, dtype=torch.int32, device="cuda")
    sub = lambda: vo.feature_matching_subset_dev(q.data_ptr(), cap * 32, n.data_ptr(), d_sel.data_ptr(), d_nsel.data_ptr(), cap, t.data_ptr(), cap * 32,
                                                 n.data_ptr() + 4 * B, gap.data_ptr(), 1, B, cap, out.data_ptr(), cap, nout.data_ptr())
    sub(); vo.sync(); vo.profile_read()
    t0 = time.perf_counter()
    for _ in range(a.reps): sub()
    vo.sync(); ds = (time.perf_counter() - t0) / a.reps
    pr = vo.profile_read()
    print("subset %5.1f %% (%d of %d rows)  %.3f ms/call  (%.2f x the unmasked call)  kernels %s"
          % (pct, k, N, ds * 1e3, ds / dt, {kk: round(v[0] / a.reps, 4) for kk, v in sorted(pr.items(), key=lambda kv: -kv[1][0])}))
vo.close()
