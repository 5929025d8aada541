"""Micro-benchmark of the chained BA (KeyframePipeline(ba_chain=True), vslam_ba_chain_dev; not part of bench.py): what running the windows of a
sequence one after another costs against the independent launch, by how many sequences the batch holds.

At B keyframes per batch (default 1024), one batch in flight, device-resident inputs, in the "reference" configuration of DESIGN.md 5.3
(pose_inputs="map", keyframe_gate="per_pass", f2f_queries="features", rejected_frames="recover", window_policy="reference", pose="lm", pose_passes=3:
its gate and its Lost rule leave few windows with keyframes, so it mostly shows what a step costs when little runs) and in the "default" one
(ba_windows="tracks" alone: every frame a keyframe, sliding windows of 10, so every step runs full windows),
for the layouts 1 x B, 16 x B/16, 64 x B/64 and 20 x 50 + rest:
  * stage_ba (window build + BA) in milliseconds with ba_chain off, and on with min_kf = 10 and min_kf = 1; the front end runs once per layout, the
    three variants are timed on the same pose-stage outputs, profiler off, after a warm-up each: whole calls until --min-seconds have passed (at least
    one), the median over --windows such windows with its range;
  * per variant one further call under the stage profiler: the milliseconds of the chain's own kernels (ba_chain_kernels: offsets + gather, scatter),
    of the BA kernels (lm_window_kernel + pose_only_wave_kernel families as the library brackets them) and of the window builder;
  * steps, windows that ran, and the ratio chain kernels / BA kernels.
Every segment of a length shows the same rendered clip.  One JSON line per record; --out FILE also writes the list.
Usage: python tools/bench_ba_chain.py [--B 1024] [--anms 1500] [--modes reference default] [--windows 3] [--min-seconds 0.3] [--layouts 1 16 64 50] [--out profiles/ba_chain.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REFERENCE_MODE = dict(pose="lm", pose_inputs="map", keyframe_gate="per_pass", f2f_queries="features", rejected_frames="recover", window_policy="reference",
                      pose_passes=3)


def _timed(p, min_seconds):
    """whole stage_ba calls until min_seconds have passed -> milliseconds per call"""
    p.vo.sync()
    t0 = time.perf_counter(); n = 0
    while True:
        p.stage_ba(); n += 1
        p.vo.sync()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return 1e3 * dt / n


def _profiled(p):
    p.vo.sync(); p.vo.profile_enable(True); p.vo.profile_read()
    p.stage_ba()
    prof = p.vo.profile_read()
    p.vo.profile_enable(False)
    ms = lambda k: round(prof.get(k, (0.0, 0, 0))[0], 3)
    return dict(chain_kernels_ms=ms("ba_chain_kernels"), ba_kernels_ms=ms("lm_window_kernel"), build_windows_ms=ms("build_windows_kernels"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--anms", type=int, default=1500)
    ap.add_argument("--unique-frames", type=int, default=64)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--layouts", nargs="+", default=["1", "16", "64", "50"], help="segments per batch; 50 = 20 clips of 50 frames + the rest")
    ap.add_argument("--modes", nargs="+", default=["reference", "default"], choices=["reference", "default"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from stereo_visual_slam_amd import synth
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = args.B
    assert B % 64 == 0 and B >= 128
    clip = synth.stereo_sequence(args.unique_frames, seed=0, workers=8)
    rest = B - 20 * 50
    shapes = {"1": ("1x%d" % B, [B]), "16": ("16x%d" % (B // 16), [B // 16] * 16), "64": ("64x%d" % (B // 64), [B // 64] * 64),
              "50": ("20x50+%d" % rest, [50] * 20 + ([rest] if rest > 0 else []))}
    n_u = lambda m: max(2, min(args.unique_frames, m)) if m > 1 else 1
    records = []
    for mode, key in [(m, k) for m in args.modes for k in args.layouts]:
        name, seg = shapes[key]
        p = KeyframePipeline(B, anms_num=args.anms, unique_frames=args.unique_frames, seed=0, ba_windows="tracks", segments=seg,
                             segment_sequences=[clip[:n_u(m)] for m in seg], ba_chain=True, **(REFERENCE_MODE if mode == "reference" else {}))
        try:
            p.stage_orb(); p.stage_stereo_match(); p.stage_track(); p.vo.sync()
            ids = p.ba_lm_id.data_ptr()
            for variant, min_kf in (("independent", None), ("chain", 10), ("chain", 1)):
                p.ba_chain = min_kf is not None
                if p.ba_chain:
                    p.ba_chain_min_kf = min_kf
                    p.vo.set_window_ids(ids, p.lm_capacity)
                else:
                    p.vo.set_window_ids(None)   # (the independent launch as every other configuration runs it: the builder writes no ids)
                p.stage_ba(); p.vo.sync()   # warm-up (the scratch grows here)
                ms = [_timed(p, args.min_seconds) for _ in range(args.windows)]
                rec = dict(mode=mode, layout=name, segments=len(seg), steps=max(seg), variant=variant, min_kf=min_kf, B=B,
                           stage_ba_ms=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3))
                rec.update(_profiled(p))
                nkf = p.ba_nkf.cpu().numpy()
                rec["windows_with_keyframes"] = int((nkf > 0).sum())
                rec["windows_ran"] = int(p.ba_ran.cpu().numpy().sum()) if p.ba_chain else int((nkf > 0).sum())
                if p.ba_chain and rec["ba_kernels_ms"] > 0:
                    rec["chain_over_ba"] = round(rec["chain_kernels_ms"] / rec["ba_kernels_ms"], 4)
                records.append(rec)
                print(json.dumps(rec), flush=True)
        finally:
            p.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="tools/bench_ba_chain.py", B=B, anms=args.anms, windows=args.windows, min_seconds=args.min_seconds, reference_mode=REFERENCE_MODE,
                           records=records), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
