#!/usr/bin/env python3
"""micro-benchmark: SGBM disparity stage only (B stereo pairs, device-resident), for kernel tuning.
Without any of the StereoSGBM options the call is the reference's fixed entry (the old code path); with one, the set goes through
vslam_disparity_map_ex_dev.  --json appends one result line to a file.
--windows N is the end-to-end protocol of profiles/sgbm_params.json: 3 warm-up calls, then N timed windows of --reps calls each with the stage
profiler off, host clock around calls that end in a synchronise; every window, their median and a checksum of the output are printed and stored."""
import argparse, hashlib, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import stereo_visual_slam_amd as pkg
from stereo_visual_slam_amd import synth
ap = argparse.ArgumentParser(); ap.add_argument("--batch", type=int, default=8); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--unique", type=int, default=2)
FIELDS = (("num_disparities", "--num-disparities"), ("block_size", "--block"), ("P1", "--p1"), ("P2", "--p2"), ("disp12_max_diff", "--disp12-max-diff"),
          ("pre_filter_cap", "--pre-filter-cap"), ("uniqueness_ratio", "--uniqueness"), ("speckle_window_size", "--speckle-window"),
          ("speckle_range", "--speckle-range"))
for f, opt in FIELDS:
    ap.add_argument(opt, dest=f, type=int, default=None)
ap.add_argument("--json", default=None, help="append the result as one JSON line to this file")
ap.add_argument("--label", default="")
ap.add_argument("--windows", type=int, default=0, help="N timed windows of --reps calls each, profiler off (0 = one profiled window)")
a = ap.parse_args()
given = {f: getattr(a, f) for f, _ in FIELDS if getattr(a, f) is not None}
sgbm = None
if given:
    if "block_size" in given:  # OpenCV's recommended penalties follow the window unless they are given too
        given.setdefault("P1", 8 * given["block_size"] ** 2); given.setdefault("P2", 32 * given["block_size"] ** 2)
    sgbm = pkg.default_sgbm_params(**given)
    pkg.sgbm_params_check(sgbm, synth.W_KITTI, synth.H_KITTI)
w, h, pitch = synth.W_KITTI, synth.H_KITTI, 1280
seq = synth.stereo_sequence(a.unique, seed=0)
buf = np.zeros((2, a.batch, h, pitch), np.uint8)
for b in range(a.batch):
    L, R = seq[b % a.unique][:2]
    buf[0, b, :, :w] = L; buf[1, b, :, :w] = R
vo = pkg.VO(device=0, max_batch=1)
d = torch.from_numpy(buf).cuda()
out = torch.empty((a.batch, h, w), dtype=torch.float32, device="cuda")
if sgbm is None:
    run = lambda: vo.disparity_map_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, a.batch, out.data_ptr())
else:
    run = lambda: vo.disparity_map_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, a.batch, out.data_ptr(), sgbm=sgbm)
if a.windows > 0:
    for _ in range(3): run()
    vo.sync()
    win = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.reps): run()
        vo.sync(); win.append(round((time.perf_counter() - t0) / a.reps * 1e3, 4))
    med = statistics.median(win)
    digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
    print("B=%d  windows ms %s  median %.4f ms  %.5f ms/pair  device MB %.0f  output %s" % (a.batch, win, med, med / a.batch, vo.device_bytes / 1e6, digest))
    if a.json:
        rec = dict(label=a.label, batch=a.batch, reps=a.reps, sgbm=list(sgbm.as_tuple()) if sgbm is not None else "reference set, fixed entry",
                   windows_ms=win, ms_per_call=med, ms_per_pair=round(med / a.batch, 5), device_mb=round(vo.device_bytes / 1e6, 1), output_sha256_16=digest)
        with open(a.json, "a") as f:
            f.write(json.dumps(rec) + "\n")
    vo.close()
    sys.exit(0)
run(); vo.sync()
vo.profile_enable(True); vo.profile_read()
t0 = time.perf_counter()
for _ in range(a.reps): run()
vo.sync(); dt = (time.perf_counter() - t0) / a.reps
pr = vo.profile_read()
D = sgbm.num_disparities if sgbm is not None else 96
print("B=%d  %.3f ms  %.1f pairs/s  %.3f ms/pair  device MB %.0f" % (a.batch, dt * 1e3, a.batch / dt, dt * 1e3 / a.batch, vo.device_bytes / 1e6))
print({k: round(v[0] / a.reps, 3) for k, v in sorted(pr.items(), key=lambda kv: -kv[1][0])})
print("valid fraction", float((out[:, :, D:] >= 0).float().mean()))
if a.json:
    rec = dict(label=a.label, batch=a.batch, reps=a.reps, sgbm=list(sgbm.as_tuple()) if sgbm is not None else "reference set, fixed entry",
               ms_per_call=round(dt * 1e3, 4), ms_per_pair=round(dt * 1e3 / a.batch, 5), device_mb=round(vo.device_bytes / 1e6, 1),
               kernels_ms={k: round(v[0] / a.reps, 3) for k, v in pr.items()})
    with open(a.json, "a") as f:
        f.write(json.dumps(rec) + "\n")
vo.close()
