"""Micro-benchmark of segmented batches (KeyframePipeline(segments=...), vslam_set_segments; not part of bench.py): many short recordings in ONE
large batch against the same recordings as lone small batches.

At B keyframes per batch (default 1024), one batch in flight, device-resident inputs, ba_windows="tracks", for the default configuration and for the
full reference mode (pose_inputs="map", keyframe_gate="per_pass", f2f_queries="features", rejected_frames="recover", window_policy="reference",
pose="lm", pose_passes=3):
  * the layouts 1 x B without a table and 1 x B with one (the same kernels: their timing windows are ALTERNATED), 4 x B/4, 16 x B/16, 20 x 50 + rest,
    64 x B/64: keyframes/s and the stage profiler's build_windows_kernels milliseconds per step;
  * the same clips as lone batches of 50, B/16 and B/64 frames, one pipeline at a time: keyframes/s.
Rates: the profiler off, a warm-up per shape, the median of --windows timing windows of at least --min-seconds each (their spread is reported).
Every segment of a length shows the same rendered clip (one rendering of --unique-frames frames serves all shapes): the work per keyframe does not
depend on which clip it is.  One JSON line per record; --out FILE also writes the list.
Usage: python tools/bench_segments.py [--B 1024] [--anms 1500] [--modes default reference] [--windows 5] [--min-seconds 0.2] [--out profiles/segments.json]"""
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


def _window(p, min_seconds):
    """one timing window: whole steps until min_seconds have passed -> keyframes/s"""
    p.vo.sync()
    t0 = time.perf_counter(); n = 0
    while True:
        p.step(); n += 1
        if n % 2 == 0 or p.B >= 256:   # (small batches: the queue is a few steps deep before the clock is read)
            p.vo.sync()
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                return p.B * n / dt


def _builder_ms(p, reps=3):
    """the stage profiler's build_windows_kernels milliseconds per step"""
    p.vo.sync(); p.vo.profile_enable(True); p.vo.profile_read()
    for _ in range(reps):
        p.step()
    prof = p.vo.profile_read()
    p.vo.profile_enable(False)
    return prof.get("build_windows_kernels", (0.0, 0, 0))[0] / reps


def _summary(rates):
    return dict(keyframes_per_s=round(float(np.median(rates)), 1), min=round(float(min(rates)), 1), max=round(float(max(rates)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--anms", type=int, default=1500)
    ap.add_argument("--unique-frames", type=int, default=64)
    ap.add_argument("--modes", nargs="+", default=["default", "reference"], choices=["default", "reference"])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from stereo_visual_slam_amd import synth
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = args.B
    assert B % 64 == 0 and B >= 128
    clip = synth.stereo_sequence(args.unique_frames, seed=0, workers=8)
    rest = B - 20 * 50
    layouts = [("%dx%d" % (k, B // k), [B // k] * k) for k in (4, 16)] + [("20x50+%d" % rest, [50] * 20 + ([rest] if rest > 0 else [])), ("64x%d" % (B // 64), [B // 64] * 64)]
    lone = sorted({50, B // 16, B // 64}, reverse=True)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    def make(n, mode_kw, segments=None):
        n_u = lambda m: max(2, min(args.unique_frames, m)) if m > 1 else 1
        kw = dict(anms_num=args.anms, unique_frames=args.unique_frames, seed=0, ba_windows="tracks", **mode_kw)
        if segments is None:
            return KeyframePipeline(n, sequence=clip[:n_u(n)], **kw)
        return KeyframePipeline(n, segments=segments, segment_sequences=[clip[:n_u(m)] for m in segments], **kw)

    for mode in args.modes:
        mode_kw = dict(REFERENCE_MODE) if mode == "reference" else {}
        # 1 x B with and without a table: the same kernels, so the two pipelines' windows alternate and each reports its own spread
        pair = [make(B, mode_kw), make(B, mode_kw, [B])]
        try:
            for p in pair:
                p.step(); p.step(); p.vo.sync()
            rates = ([], [])
            for _ in range(args.windows):
                for i, p in enumerate(pair):
                    rates[i].append(_window(p, args.min_seconds))
            for i, p in enumerate(pair):
                emit(dict(mode=mode, layout="1x%d" % B, table=bool(i), B=B, build_windows_ms=round(_builder_ms(p), 3), **_summary(rates[i])))
        finally:
            for p in pair:
                p.close()
        for name, seg in layouts:
            p = make(B, mode_kw, seg)
            try:
                p.step(); p.step(); p.vo.sync()
                r = [_window(p, args.min_seconds) for _ in range(args.windows)]
                emit(dict(mode=mode, layout=name, table=True, B=B, segments=len(seg), build_windows_ms=round(_builder_ms(p), 3), **_summary(r)))
            finally:
                p.close()
        for n in lone:   # the same clips as lone batches, one pipeline at a time
            p = make(n, mode_kw)
            try:
                for _ in range(4):
                    p.step()
                p.vo.sync()
                r = [_window(p, args.min_seconds) for _ in range(args.windows)]
                emit(dict(mode=mode, layout="lone %d" % n, table=False, B=n, build_windows_ms=round(_builder_ms(p), 3), **_summary(r)))
            finally:
                p.close()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(dict(tool="tools/bench_segments.py", B=B, anms=args.anms, windows=args.windows, min_seconds=args.min_seconds, records=records), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
