"""Time the device window builder (vslam_build_windows_dev / vslam_build_windows_kf_dev / vslam_build_windows_gated_dev) under both keyframe
policies and with the keyframe gate, and the BA schedule on the windows each one builds.

Cases (B = --batch keyframes each):
  bench       the bench's rendered sequence (one pipeline, seed 0, unique_frames = B, ping-pong over it, anms 1500, L/R match depth);
  stationary  one rendered frame repeated B times: tracks about B frames long, every pose near every other (the near-eviction branch
              every step, old keyframes kept).
Per case and policy: the builder's time (median of --reps, CUDA events on the pipeline's stream), the BA schedule's time on its windows, how
many steps evicted something other than the oldest keyframe, and the ATE (RMS camera-centre error against the rendered ground truth, both in
frame 0's world) of the trajectory from the BA windows next to that of the chained pose-stage poses.  "gated" is the culled build with
insert_key_frame's keyframe gate: it also reports the keyframe fraction and the rejected frames, and its ATE is over the keyframes it writes.
Prints one JSON line.
Kernel-level split (the serial kf_set_kernel's share of the culled build): run this under `rocprofv3 --kernel-trace --stats -- python ...`
in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _centres(T):
    from stereo_visual_slam_amd.synth import R_from_quat
    return np.array([-R_from_quat(t[:4] / np.linalg.norm(t[:4])).T @ t[4:] for t in T])


def _chain(T_rel):
    """G[f] = T_rel[f - 1] o G[f - 1], in numpy (for the report, not a parity check)"""
    from stereo_visual_slam_amd.synth import R_from_quat, quat_from_R
    G = [np.array([0, 0, 0, 1, 0, 0, 0], np.float64)]
    for T in T_rel:
        Ra, Rb = R_from_quat(T[:4] / np.linalg.norm(T[:4])), R_from_quat(G[-1][:4])
        G.append(np.concatenate([np.asarray(quat_from_R(Ra @ Rb), np.float64), Ra @ G[-1][4:] + T[4:]]))
    return np.stack(G)


def _time(pipe, fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(pipe.stream):
            a.record()
        fn()
        with torch.cuda.stream(pipe.stream):
            b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def run_case(name, pipe, gt, reps):
    import torch
    from stereo_visual_slam_amd.trajectory import sliding_keyframes
    pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track()
    torch.cuda.synchronize()
    B = pipe.B
    res = dict(case=name, B=B)
    chained = _chain(pipe.d_Tpnp.cpu().numpy()[:B - 1])
    gt_c = _centres(gt)
    res["ate_chained_m"] = float(np.sqrt(np.mean(np.sum((_centres(chained) - gt_c) ** 2, 1))))
    for policy in ("sliding", "reference", "gated"):
        pipe.window_policy = "reference" if policy == "gated" else policy
        pipe.keyframe_gate = policy == "gated"
        pipe.stage_build_windows()   # (warm: the scratch is allocated on the first call of a policy)
        torch.cuda.synchronize()
        t_build, all_build = _time(pipe, pipe.stage_build_windows, reps)
        torch.cuda.synchronize()
        built = dict(ba_build_status=pipe.ba_build_status.cpu().numpy(), ba_lm_off=pipe.ba_lm_off.cpu().numpy(), ba_e_off=pipe.ba_e_off.cpu().numpy())
        if policy != "sliding":
            built["ba_kf_frame"], built["ba_evicted"] = pipe.ba_kf_frame.cpu().numpy(), pipe.ba_evicted.cpu().numpy()
        else:
            built["ba_kf_frame"], built["ba_evicted"] = sliding_keyframes(B, pipe.n_kf)
        assert (built["ba_build_status"][0] & 3) == 0, (name, policy, built["ba_build_status"])
        T0 = pipe.ba_T.clone()

        def ba():
            with torch.cuda.stream(pipe.stream):
                pipe.ba_T.copy_(T0); pipe.ba_inl.fill_(1)
            pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        t_ba, _ = _time(pipe, ba, max(1, reps // 3))
        ids, T = pipe.trajectory()
        ev, kf = built["ba_evicted"], built["ba_kf_frame"]
        order = np.argsort(ids)
        not_oldest = int(sum(1 for b in range(1, B) if ev[b] >= 0 and ev[b] != kf[b - 1][0]))
        res[policy] = dict(build_ms=round(t_build, 4), build_ms_all=[round(x, 4) for x in all_build], ba_schedule_ms=round(t_ba, 3),
                           landmarks=int(built["ba_lm_off"][B]), edges=int(built["ba_e_off"][B]), evicted_not_oldest=not_oldest,
                           oldest_member_age_max=int(max(b - kf[b][0] for b in range(B))),
                           ate_m=float(np.sqrt(np.mean(np.sum((_centres(T[order]) - gt_c[ids[order]]) ** 2, 1)))))
        if policy == "gated":
            st = pipe.ba_frame_state.cpu().numpy()
            res[policy].update(keyframes=int((st == 2).sum()), keyframe_fraction=round(float((st == 2).mean()), 4), tracked=int((st == 1).sum()),
                               rejected=int((st == 0).sum()), status=int(built["ba_build_status"][0]),
                               ate_chained_keyframes_m=float(np.sqrt(np.mean(np.sum((_centres(chained[ids[order]]) - gt_c[ids[order]]) ** 2, 1)))))
    res["culled_over_sliding_build"] = round(res["reference"]["build_ms"] / res["sliding"]["build_ms"], 3)
    res["gated_over_culled_build"] = round(res["gated"]["build_ms"] / res["reference"]["build_ms"], 3)
    res["gated_over_culled_ba"] = round(res["gated"]["ba_schedule_ms"] / res["reference"]["ba_schedule_ms"], 3)
    pipe.keyframe_gate = False
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cases", default="bench,stationary")
    ap.add_argument("--render-workers", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    from stereo_visual_slam_amd import synth
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = args.batch
    results = []
    t0 = time.time()
    seq = synth.stereo_sequence(B, seed=0, workers=args.render_workers)
    for case in args.cases.split(","):
        if case == "bench":
            pipe = KeyframePipeline(B, anms_num=1500, unique_frames=B, seed=0, sequence=seq, ba_windows="tracks", window_policy="reference",
                                    keyframe_gate=True)
            gt = [seq[f][2] for f in pipe.frame_of]
        elif case == "stationary":
            pipe = KeyframePipeline(B, anms_num=1500, unique_frames=2, seed=0, sequence=[seq[0], seq[0]], ba_windows="tracks", window_policy="reference",
                                    keyframe_gate=True)
            gt = [seq[0][2]] * B
        else:
            raise SystemExit("unknown case %r" % case)
        try:
            results.append(run_case(case, pipe, gt, args.reps))
        finally:
            pipe.close()
        print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    line = json.dumps(dict(tool="bench_windows", batch=B, reps=args.reps, wall_s=round(time.time() - t0, 1), results=results))
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
