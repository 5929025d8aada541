"""Micro-benchmark of the rectification stage (vslam_rectify_dev): ms per call at B stereo pairs, 1392 x 512 raw -> 1241 x 376 rectified, rig
"kitti_raw_like" of tests/rectify_ref.py, against the library's own streaming copy (vslam_hbm_copy_probe) moving the stage's compulsory
bytes -- one read of every source image, one write of every destination image -- in the same process.

    python tools/bench_rectify.py [--batches 1,32,256,1024] [--form gather,lds] [--windows 5] [--out profiles/rectify.json]

--form: the source side of the kernel (vslam_set_tuning "rectify_form"): "gather" = direct byte gathers through the vector cache, "lds" = every
tile's source box staged in LDS; both by default, and "default" = whatever the library picks.

A figure is the median of `--windows` timed windows, each a host clock around enough back-to-back calls to last >= 0.2 s, ending in a
synchronise.  Outputs are checked against the numpy restatement on the first image of each side before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rectify_ref as RR  # noqa: E402
import stereo_visual_slam_amd as pkg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32,256,1024")
    ap.add_argument("--form", default="gather,lds")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rig", default="kitti_raw_like")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rectify: no GPU visible (there is nothing to measure without one)")
    rig = RR.RIGS[a.rig]
    (sw, sh), (w, h) = rig["src"], rig["dst"]
    sp, dp = (sw + 63) // 64 * 64, (w + 63) // 64 * 64
    params = RR.params_of(pkg, a.rig)
    maps = [pkg.rectify_build_maps(params, s, w, h) for s in (0, 1)]
    res = dict(rig=a.rig, src=[sw, sh], dst=[w, h], src_pitch=sp, dst_pitch=dp, windows=a.windows, device=torch.cuda.get_device_name(0), cases=[])
    rng = np.random.default_rng(0)
    forms = {"gather": 0, "lds": 1, "default": -1}
    for B, form in [(int(b), f) for b in a.batches.split(",") for f in a.form.split(",")]:
        vo = pkg.VO(device=0, max_batch=B, img_w=w, img_h=h)
        try:
            vo.set_tuning(rectify_form=forms[form])
            vo.rectify_set(params)
            # B images per side from 8 distinct noise images (the gather's cost does not depend on the pixel values)
            base = torch.from_numpy(rng.integers(0, 256, (2, 8, sh, sp)).astype(np.uint8)).cuda()
            src = base[:, torch.arange(B, device="cuda") % 8].contiguous()
            dst = torch.zeros((2, B, h, dp), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            call = lambda: vo.rectify_dev(src[0].data_ptr(), src[1].data_ptr(), sh * sp, sp, B, dst[0].data_ptr(), dst[1].data_ptr(), h * dp, dp)
            call(); vo.sync()
            for s in (0, 1):
                want = RR.remap(src[s, 0, :, :sw].cpu().numpy(), *maps[s])
                got = dst[s, 0].cpu().numpy()
                assert np.array_equal(got[:, :w], want) and not got[:, w:].any(), "rectify_dev differs from the restatement"
                assert torch.equal(dst[s, B - 1], dst[s, (B - 1) % 8]), "last image of the batch differs from its twin"
            t0 = time.perf_counter(); n = 0
            while time.perf_counter() - t0 < 0.2:   # calls per window
                call(); n += 1
            vo.sync()
            n = max(3, int(n * 0.2 / (time.perf_counter() - t0)) + 1)
            wins = []
            for _ in range(a.windows):
                vo.sync(); t0 = time.perf_counter()
                for _ in range(n):
                    call()
                vo.sync()
                wins.append((time.perf_counter() - t0) * 1e3 / n)
            ms = float(np.median(wins))
            nbytes = 2 * B * (sp * sh + dp * h)
            gbs = vo.hbm_copy_probe(max(nbytes // 2, 1 << 20), 20)   # a copy of nbytes / 2 moves nbytes
            copy_ms = max(nbytes, 2 << 20) / gbs * 1e-6
            case = dict(B=B, form=form, ms_per_call=round(ms, 4), ms_windows=[round(x, 4) for x in wins], calls_per_window=n, us_per_pair=round(ms * 1e3 / B, 3),
                        compulsory_bytes=nbytes, compulsory_gbs=round(nbytes / ms * 1e-6, 1), copy_probe_gbs=round(gbs, 1),
                        copy_probe_ms_same_bytes=round(copy_ms, 4), ratio_to_copy=round(ms / copy_ms, 2))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
        finally:
            vo.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
