"""Micro-benchmark of the pose stage against the map (KeyframePipeline(pose_inputs="map"); not part of bench.py).

Per pose solver: one B-keyframe batch of rendered frames through stage A (own-depth inputs) and through K = 1, 2, 4 refinement passes.  Reports
  * ms per pass: the stage profiler's kernel time of stage_track with K passes, minus stage A's, over K (the passes' input builds, chain and
    solver launches; the few torch ops between them are not bracketed);
  * pose inputs per frame: stage A's (matches whose last-frame keypoint owns a depth) and pass 1's (every match out of a feature);
  * pose error against the rendered ground truth (synth.stereo_sequence's T_c_w, taken relative to the batch's first frame): translation and
    rotation error of every frame's absolute pose -- stage A's chained relative poses for "own_depth", G^K for "map".
Usage: python tools/bench_pose_map.py [--B 1024] [--pose lm ransac] [--passes 1 2 4] [--reps 3]; one JSON line per configuration."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rot(T):
    x, y, z, w = T[:4]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _mat(T):
    M = np.eye(4)
    M[:3, :3] = _rot(T); M[:3, 3] = T[4:7]
    return M


def pose_errors(G, gt):
    """G, gt: (B, 4, 4) T_c_w with frame 0 as the world; per frame (translation error of the camera centre in m, rotation error in rad)"""
    te, re = [], []
    for A, Bm in zip(G, gt):
        D = A @ np.linalg.inv(Bm)
        te.append(float(np.linalg.norm(np.linalg.inv(A)[:3, 3] - np.linalg.inv(Bm)[:3, 3])))
        re.append(float(math.acos(max(-1.0, min(1.0, (np.trace(D[:3, :3]) - 1) / 2)))))
    return np.array(te), np.array(re)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--pose", nargs="+", default=["lm", "ransac"], choices=["lm", "ransac"])
    ap.add_argument("--passes", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--unique-frames", type=int, default=64)
    args = ap.parse_args()
    import torch
    from stereo_visual_slam_amd import synth
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = args.B
    seq = synth.stereo_sequence(min(args.unique_frames, B), seed=0, workers=8)
    for pose in args.pose:
        base_ms = None
        for K in [0] + list(args.passes):
            kw = dict(pose_inputs="map", pose_passes=K) if K else {}
            p = KeyframePipeline(B, unique_frames=len(seq), sequence=seq, ba_windows="tracks", pose=pose, **kw)
            try:
                p.stage_orb(); p.stage_stereo_match()
                p.stage_track()                     # (warm-up: scratch growth, first launches)
                p.vo.sync(); p.vo.profile_enable(True); p.vo.profile_read()
                fam = {}
                for _ in range(args.reps):
                    p.stage_track()
                    for k, (ms, _, _) in p.vo.profile_read().items():
                        fam[k] = fam.get(k, 0.0) + ms / args.reps
                p.vo.profile_enable(False)
                out = p.download()
                if K:
                    G = out["T_c_w"]
                else:
                    dG = torch.zeros((B, 7), dtype=torch.float64, device=p.dev)
                    p.vo.chain_poses_dev(B, p.d_Tpnp.data_ptr(), dG.data_ptr()); p.vo.sync()
                    G = dG.cpu().numpy()
                gt = np.stack([_mat(seq[f][2]) for f in p.frame_of])
                gt = gt @ np.linalg.inv(gt[0])[None]
                te, re = pose_errors(np.stack([_mat(g) for g in G]), gt)
                rec = dict(pose=pose, mode="map" if K else "own_depth", passes=K, B=B, stage_track_kernel_ms=round(sum(fam.values()), 3),
                           families={k: round(v, 3) for k, v in sorted(fam.items())},
                           inputs_per_frame_stage_a=round(float(out["pn"][:B - 1].mean()), 1),
                           matches_per_frame=round(float(out["nf2f"][:B - 1].mean()), 1),
                           trans_err_m=dict(mean=round(float(te.mean()), 3), median=round(float(np.median(te)), 3), max=round(float(te.max()), 3)),
                           rot_err_rad=dict(mean=round(float(re.mean()), 5), max=round(float(re.max()), 5)))
                if not K:
                    base_ms = rec["stage_track_kernel_ms"]
                else:
                    rec["ms_per_pass"] = round((rec["stage_track_kernel_ms"] - base_ms) / K, 3)
                    rec["inputs_per_frame_map"] = round(float(out["map_n"][:B - 1].mean()), 1)
                    rec["items_without_model"] = int((out["map_ninl"][:B - 1] == 0).sum())
                print(json.dumps(rec), flush=True)
            finally:
                p.close()


if __name__ == "__main__":
    main()
