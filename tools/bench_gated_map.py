"""Micro-benchmark of the keyframe gate inside the map-based pose passes (KeyframePipeline(pose_inputs="map", keyframe_gate="per_pass"); not part of
bench.py).

Per pose solver, one B-keyframe batch of rendered frames through
  * stage A with the gate on its own-depth inputs (keyframe_gate=True): the keyframes it selects;
  * K = 1, 2, 4 and B - 1 refinement passes without the gate (keyframe_gate=False) and with it (keyframe_gate="per_pass"); B - 1 passes are the
    sequential loop (include/vslam_hip.h), the states every smaller K converges to from frame 0 on.
Reports, one JSON line per configuration:
  * ms per pass: the stage profiler's kernel time of stage_track with K passes, minus stage A's, over K (as tools/bench_pose_map.py), and for the
    gated passes the ratio to the ungated ones;
  * keyframes per B frames (state 2);
  * state changes from pass K - 1 to pass K (frame_state against frame_state_prev);
  * keyframe-trajectory error against the rendered ground truth: trajectory() after the BA schedule (the keyframes' BA-refined poses, each from
    the last keyframe window that held it) against synth.stereo_sequence's T_c_w, both relative to the batch's first frame.
--queries all features: the gated passes with stage A's all-keypoint frame-to-frame table ("all") and with every pair re-matched per pass on the
features of its first frame, the reference's query set (f2f_queries="features"); per record also the mean pose inputs per frame of the last pass.
--rejected pass_through recover: the feature-query passes as they are ("pass_through": a rejected frame is treated like a tracked one) and with the
reference's failure handling (rejected_frames="recover": a rejected frame is dropped and the next one matched against the last accepted frame at
the real frame gap; needs --queries features); per record also the Lost frames and the largest gap of the last pass's pairing.
--noise-share S: that share of the rendered frames (every round(1 / S)-th, never frame 0) has both images replaced by synth.noise_image, so that
the pose stage rejects them: the input on which the two modes differ.  --kernels: the stage profiler's milliseconds per kernel family of one step.
Usage: python tools/bench_gated_map.py [--B 1024] [--pose lm ransac] [--passes 1 2 4 -1] [--reps 3] [--queries all features]
                                       [--rejected pass_through recover] [--noise-share 0.05] [--kernels]   (-1: B - 1 passes)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pose_map import _mat, pose_errors  # noqa: E402


def _track_ms(p, reps, kernels=None):
    """kernel milliseconds of one stage_track (mean of reps, after a warm-up); kernels (a dict): filled with the mean per kernel family"""
    p.stage_track()
    p.vo.sync(); p.vo.profile_enable(True); p.vo.profile_read()
    tot = 0.0
    for _ in range(reps):
        p.stage_track()
        prof = p.vo.profile_read()
        tot += sum(ms for ms, _, _ in prof.values())
        if kernels is not None:
            for name, (ms, _, _) in prof.items():
                kernels[name] = kernels.get(name, 0.0) + ms / reps
    p.vo.profile_enable(False)
    return tot / reps


def _kf_errors(p, seq):
    """the BA schedule on the step's windows, then trajectory(): per keyframe (translation error in m, rotation error in rad) against the rendering"""
    p.stage_build_windows()
    p.vo.ba_batch_dev(p.ba_batch, schedule=1)
    ids, T = p.trajectory()
    gt = np.stack([_mat(seq[f][2]) for f in p.frame_of])
    gt = gt @ np.linalg.inv(gt[0])[None]
    te, re = pose_errors(np.stack([_mat(t) for t in T]), gt[ids])
    return len(ids), te, re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--pose", nargs="+", default=["lm", "ransac"], choices=["lm", "ransac"])
    ap.add_argument("--passes", nargs="+", type=int, default=[1, 2, 4, -1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--unique-frames", type=int, default=64)
    ap.add_argument("--queries", nargs="+", default=["all"], choices=["all", "features"])
    ap.add_argument("--rejected", nargs="+", default=["pass_through"], choices=["pass_through", "recover"])
    ap.add_argument("--noise-share", type=float, default=0.0)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    assert "recover" not in args.rejected or "features" in args.queries, "--rejected recover needs --queries features"
    from stereo_visual_slam_amd import synth
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = args.B
    seq = synth.stereo_sequence(min(args.unique_frames, B), seed=0, workers=8)
    noise = []
    if args.noise_share > 0:   # planted rejected frames: nothing in a noise image matches its neighbours
        seq = list(seq)
        noise = list(range(max(1, int(round(0.5 / args.noise_share))), len(seq), max(2, int(round(1.0 / args.noise_share)))))
        for f in noise:
            seq[f] = (synth.noise_image(100 + f), synth.noise_image(200 + f)) + tuple(seq[f][2:])
    for pose in args.pose:
        base_ms, ungated_ms = None, {}
        configs = [("stage_a", 0, "all", "pass_through")] + [(g, K if K > 0 else B - 1, qs, rj) for K in args.passes for g in ("ungated", "per_pass")
                                                             for qs in (args.queries if g == "per_pass" else ["all"])
                                                             for rj in (args.rejected if g == "per_pass" and qs == "features" else ["pass_through"])]
        for gate, K, queries, rejected in configs:
            kw = dict(keyframe_gate=True) if gate == "stage_a" else dict(pose_inputs="map", pose_passes=K,
                                                                         keyframe_gate="per_pass" if gate == "per_pass" else False)
            if queries != "all":
                kw["f2f_queries"] = queries
            if rejected != "pass_through":
                kw["rejected_frames"] = rejected
            p = KeyframePipeline(B, unique_frames=len(seq), sequence=seq, ba_windows="tracks", pose=pose, window_policy="reference", **kw)
            try:
                p.stage_orb(); p.stage_stereo_match()
                kernels = {} if args.kernels else None
                ms = _track_ms(p, args.reps, kernels)
                rec = dict(pose=pose, gate=gate, queries=queries, rejected_frames=rejected, passes=K, B=B, noise_frames=len(noise),
                           stage_track_kernel_ms=round(ms, 3))
                if kernels is not None:
                    rec["kernel_ms"] = {k: round(v, 4) for k, v in sorted(kernels.items())}
                if gate == "stage_a":
                    base_ms = ms
                else:
                    rec["ms_per_pass"] = round((ms - base_ms) / K, 3)
                    if gate == "ungated":
                        ungated_ms[K] = rec["ms_per_pass"]
                    elif ungated_ms.get(K):
                        rec["gated_over_ungated"] = round(rec["ms_per_pass"] / ungated_ms[K], 3)
                if gate != "ungated":
                    n, te, re = _kf_errors(p, seq)   # (stage A's gate runs in the window build: its states exist from here on)
                    out = p.download()
                    st = out["frame_state"]
                    rec["keyframes"] = int((st == 2).sum()); rec["rejected"] = int((st == 0).sum())
                    rec["keyframes_per_1024"] = round(1024.0 * rec["keyframes"] / B, 1)
                    if gate == "per_pass":
                        rec["inputs_per_frame"] = round(float(out["map_n"][:B - 1].mean()), 1)
                        rec["inliers_per_frame"] = round(float(out["map_ninl"][:B - 1].mean()), 1)
                        rec["state_changes_last_pass"] = int((st != out["frame_state_prev"]).sum())
                    if rejected == "recover":
                        rec["lost"] = int((st == 3).sum()); rec["max_gap"] = float(out["map_gap"][:B - 1].max())
                    rec["trajectory_keyframes"] = n
                    rec["kf_trans_err_m"] = dict(mean=round(float(te.mean()), 4), median=round(float(np.median(te)), 4), max=round(float(te.max()), 4))
                    rec["kf_rot_err_rad"] = dict(mean=round(float(re.mean()), 5), max=round(float(re.max()), 5))
                    rec["ba_status_nonzero"] = int((p.vo.ba_status(B)[st == 2] != 0).sum())
                print(json.dumps(rec), flush=True)
            finally:
                p.close()


if __name__ == "__main__":
    main()
