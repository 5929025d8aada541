"""Micro-benchmark of match by projection (vslam_project_match_dev): ms per call for M items x L landmarks against images of N keypoints, beside the
time a streaming copy (vslam_hbm_copy_probe) needs for the call's compulsory bytes.

    python tools/bench_project_match.py [--items 1024] [--landmarks 5000] [--keypoints 1500] [--images 64] [--windows 5] [--out profiles/project_match.json]

Keypoints are uniform over 1241 x 376 on a quarter-pixel lattice; every landmark is the back-projection (identity pose, depth 5 .. 60) of a keypoint
of its item's image moved by up to +-3 px (lattice + 0.125), and carries that keypoint's descriptor with 0 .. 60 bits flipped -- its row indexes a
separate source array, as a map's descriptors would.  Items are sorted by image, M / images items per image.  Compulsory bytes: per landmark 24
(point) + 4 (row) + 32 (descriptor) in and 13 out, per item 64, per image N x (28 + 32).  A figure is the median of `--windows` timed windows, each a
host clock around enough back-to-back calls to last >= 0.2 s, ending in a synchronise; the profiler is off.  Before anything is timed a small batch
of the same make is compared with the yardstick tests/project_match_ref.py bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import project_match_ref as R  # noqa: E402
import stereo_visual_slam_amd as pkg  # noqa: E402

W, H = 1241, 376
K4 = (718.856, 718.856, 607.1928, 185.2157)


def timed(call, sync, windows):
    """median ms per call over `windows` windows of >= 0.2 s (the calls per window come from one synchronised call)"""
    call(); sync()
    t0 = time.perf_counter(); call(); sync()
    n = max(3, int(0.2 / max(time.perf_counter() - t0, 1e-6)) + 1)
    wins = []
    for _ in range(windows):
        sync(); t0 = time.perf_counter()
        for _ in range(n):
            call()
        sync()
        wins.append((time.perf_counter() - t0) * 1e3 / n)
    return float(np.median(wins)), [round(x, 4) for x in wins], n


def make(rng, M, L, N, B):
    kps = np.zeros((B, N), pkg.KEYPOINT_DTYPE)
    kps["x"] = rng.integers(0, 4 * (W - 1) + 1, (B, N)) / 4.0; kps["y"] = rng.integers(0, 4 * (H - 1) + 1, (B, N)) / 4.0
    desc = rng.integers(0, 256, (B, N, 32)).astype(np.uint8)
    img = np.sort(np.arange(M) % B).astype(np.int32)
    j = rng.integers(0, N, (M, L))
    u = kps["x"][img[:, None], j].astype(np.float64) + rng.integers(-12, 13, (M, L)) * 0.25 + 0.125
    v = kps["y"][img[:, None], j].astype(np.float64) + rng.integers(-12, 13, (M, L)) * 0.25 + 0.125
    z = rng.uniform(5, 60, (M, L))
    xyz = np.stack([(u - K4[2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z], -1).reshape(-1, 3)
    src = desc[img[:, None], j].reshape(-1, 32).copy()
    flips = rng.integers(0, 61, len(src))
    for k in range(60):   # flip bit (37 k) mod 256 of every row that asked for more than k flips
        b = (37 * k) % 256
        src[flips > k, b >> 3] ^= np.uint8(1 << (b & 7))
    T = np.tile(np.array([0, 0, 0, 1.0, 0, 0, 0]), (M, 1))
    return dict(lm_off=(np.arange(M + 1) * L).astype(np.int32), item_img=img, item_T=T, lm_xyz=xyz, lm_desc_row=np.arange(M * L, dtype=np.int32), src_desc=src,
                kps=kps, desc=desc, n=np.full(B, N, np.int32))


def check(vo):
    c = make(np.random.default_rng(1), 3, 400, 1500, 2)
    got = vo.project_match(c["lm_off"], c["item_img"], c["item_T"], c["lm_xyz"], c["lm_desc_row"], c["src_desc"], c["kps"], c["desc"], c["n"], K4=K4)
    want = R.project_match(c["lm_off"], c["item_img"], c["item_T"], c["lm_xyz"], c["lm_desc_row"], c["src_desc"], np.stack([c["kps"]["x"], c["kps"]["y"]], -1), c["desc"],
                           c["n"], K4, W, H)
    for key in ("status", "match", "dist", "n_cand"):
        assert np.array_equal(got[key], want[key]), "yardstick check: " + key
    return np.bincount(want["status"], minlength=8).tolist()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1024); ap.add_argument("--landmarks", type=int, default=5000); ap.add_argument("--keypoints", type=int, default=1500)
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--windows", type=int, default=5); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M, L, N, B = a.items, a.landmarks, a.keypoints, min(a.images, a.items)
    vo = pkg.VO(device=0, max_batch=4)
    dev = torch.device("cuda:0")
    status_check = check(vo)
    c = make(np.random.default_rng(0), M, L, N, B)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t = dict(off=up(c["lm_off"]), img=up(c["item_img"]), T=up(c["item_T"]), xyz=up(c["lm_xyz"]), row=up(c["lm_desc_row"]), src=up(c["src_desc"]),
             kps=up(c["kps"].view(np.uint8)), desc=up(c["desc"]), n=up(c["n"]))
    out = dict(match=torch.empty(M * L, dtype=torch.int32, device=dev), dist=torch.empty(M * L, dtype=torch.int32, device=dev),
               n_cand=torch.empty(M * L, dtype=torch.int32, device=dev), status=torch.empty(M * L, dtype=torch.uint8, device=dev))
    k4 = (pkg.C.c_double * 4)(*K4)
    batch = pkg.ProjectMatchBatch(n_items=M, n_landmarks=M * L, B=B, kp_capacity=N, n_src_rows=M * L, d_lm_off=t["off"].data_ptr(), d_item_img=t["img"].data_ptr(),
                                  d_item_T=t["T"].data_ptr(), d_lm_xyz=t["xyz"].data_ptr(), d_lm_desc_row=t["row"].data_ptr(), d_src_desc=t["src"].data_ptr(),
                                  d_kps=t["kps"].data_ptr(), d_desc=t["desc"].data_ptr(), desc_stride_bytes=0, d_n=t["n"].data_ptr(),
                                  K4=pkg.C.cast(k4, pkg.C.POINTER(pkg.C.c_double)), d_match=out["match"].data_ptr(), d_dist=out["dist"].data_ptr(),
                                  d_n_cand=out["n_cand"].data_ptr(), d_status=out["status"].data_ptr())
    params = pkg.default_project_match_params()
    torch.cuda.synchronize()
    call = lambda: vo.project_match_dev(batch, params)
    forms = {}
    for stage in (0, 1):   # the two forms of the kernel: candidates' descriptors from L2, or staged in LDS
        vo.set_tuning(pm_stage=stage)
        forms[stage] = timed(call, vo.sync, a.windows)
    vo.set_tuning(pm_stage=-1)
    ms, wins, n_calls = timed(call, vo.sync, a.windows)
    status = torch.bincount(out["status"].long(), minlength=8).cpu().tolist()
    n_cand = float(out["n_cand"].double().mean().item())
    nbytes = M * L * (24 + 4 + 32 + 13) + M * 64 + B * N * 60
    probe = vo.hbm_copy_probe_best()
    floor = nbytes / (probe["gbs"] * 1e9) * 1e3
    res = dict(items=M, landmarks_per_item=L, keypoints=N, images=B, radius_px=params.radius_px, tau=params.tau, ratio_pct=params.ratio_pct, ms=round(ms, 4),
               ms_descriptors_from_l2=round(forms[0][0], 4), windows_ms_from_l2=forms[0][1], ms_descriptors_in_lds=round(forms[1][0], 4), windows_ms_in_lds=forms[1][1],
               windows_ms=wins, calls_per_window=n_calls, candidates_per_landmark=round(n_cand, 3), status_counts=dict(zip(R.STATUS_NAMES, status)),
               compulsory_bytes=nbytes, hbm_copy_gbs=probe["gbs"], hbm_copy_variant=probe["variant"], copy_floor_ms=round(floor, 4),
               fraction_of_copy_floor=round(floor / ms, 4), landmarks_per_second=round(M * L / (ms * 1e-3)), lds_bytes_per_workgroup=N * 18 + 39 * 12 * 4,
               yardstick_check_status_counts=dict(zip(R.STATUS_NAMES, status_check)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    vo.close()


if __name__ == "__main__":
    main()
