"""Micro-benchmark of the dense map stage on the SGBM disparities of the rendered sequence: ms per call of vslam_voxel_fuse_disparity_dev in both
forms, of vslam_voxel_insert_points_dev on the same points (vslam_reproject_dev's), and of vslam_voxel_extract_dev, each against the library's own
streaming copy (vslam_hbm_copy_probe) moving the stage's compulsory bytes -- 4 B of disparity and 1 B of gray read per pixel -- in the same process.

    python tools/bench_voxel.py [--batches 256,1024] [--voxel 0.2] [--windows 5] [--out profiles/voxel.json]

The inputs are one KeyframePipeline(depth="sgbm", ba_windows="tracks") step at each batch size: its disparity maps, left images and BA-refined
poses (KeyframePipeline.dense_map_inputs).  Step 1, the depth gate of dense_map (depth_min, depth_reliable), a table sized for a load factor
below one half.  A figure is the median of `--windows` timed windows, each a host clock around enough back-to-back calls to last >= 0.2 s, ending
in a synchronise; the profiler is off.  "fresh" = into a table cleared before every call (the clear's own time, measured the same way, taken
off); "warm" = into the table the previous call filled (every voxel exists: no slot is claimed).  Before anything is timed, the first two frames
go through both forms and the two-stage path into a small table and are compared with the numpy restatement tests/voxel_ref.py bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voxel_ref as VR  # noqa: E402
from stereo_visual_slam_amd.pipeline import KeyframePipeline  # noqa: E402


def timed(call, sync, windows):
    """median ms per call over `windows` windows of >= 0.2 s.  The calls per window come from one synchronised call: a call lasts milliseconds and
    is enqueued in microseconds, so a host loop that enqueues for 0.2 s would queue minutes of work."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--unique-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_voxel: no GPU visible (there is nothing to measure without one)")
    res = dict(voxel_size=a.voxel, windows=a.windows, device=torch.cuda.get_device_name(0), cases=[])
    seq = None
    for B in [int(b) for b in a.batches.split(",")]:
        p = KeyframePipeline(B, anms_num=500, unique_frames=a.unique_frames, seed=0, ba_windows="tracks", depth="sgbm", sequence=seq, render_workers=8)
        try:
            seq = p.h_seq
            vo, w, h = p.vo, p.w, p.h
            p.step()
            T, map_id = p.dense_map_inputs()
            z_min, z_max = vo.params.depth_min, vo.params.depth_reliable
            with torch.cuda.stream(p.stream):
                d_T = torch.from_numpy(T).to(p.dev); d_id = torch.from_numpy(map_id).to(p.dev)
                d_gray = p.d_imgs[:B, :, :w].contiguous()                     # the two-stage path's intensities, one byte per point
                d_xyz = torch.zeros((B, h, w, 3), dtype=torch.float32, device=p.dev); d_valid = torch.zeros((B, h, w), dtype=torch.uint8, device=p.dev)
            fuse = lambda vm, n=B: vo.voxel_fuse_disparity_dev(vm, p.d_disp.data_ptr(), p.d_imgs.data_ptr(), p.img_bytes, p.pitch, w, h, n, d_T.data_ptr(),
                                                               d_id.data_ptr(), z_min, z_max, 1)
            insert = lambda vm, n=B: vo.voxel_insert_points_dev(vm, d_xyz.data_ptr(), d_valid.data_ptr(), d_gray.data_ptr(), n * h * w, 0)
            vo.reproject_dev(p.d_disp.data_ptr(), w, h, B, d_T.data_ptr(), z_min, z_max, 1, d_xyz.data_ptr(), d_valid.data_ptr())
            vo.sync()
            # ---- the check: two frames, both forms and the two-stage path against the restatement
            assert (map_id[:2] == 0).all()
            ref = VR.VoxelRef(a.voxel)
            ref.insert(d_xyz[:2].cpu().numpy().reshape(-1, 3), d_valid[:2].cpu().numpy().ravel(), d_gray[:2].cpu().numpy().ravel(), 0)
            want = ref.extract()
            small = vo.voxel_map(a.voxel, 20)
            for form, call in ((0, fuse), (1, fuse), (-1, insert)):
                vo.set_tuning(voxel_form=form)
                small.clear(); call(small, 2)
                got = small.extract()
                assert got.tobytes() == want.tobytes() and small.stats()["n_dropped_full"] == 0, "the dense map differs from the restatement (form %d)" % form
            small.close()
            # ---- the table: load factor below one half
            probe = vo.voxel_map(a.voxel, 26)
            fuse(probe)
            occ = probe.stats()["n_occupied"]
            probe.close()
            log2 = max(10, int(2 * occ).bit_length())   # the smallest table with 2^log2 > 2 x occupied
            vm = vo.voxel_map(a.voxel, log2)
            sync = vo.sync
            case = dict(B=B, log2_capacity=log2, pixels=B * h * w)
            clear_ms, _, _ = timed(vm.clear, sync, a.windows)
            case["clear_ms"] = round(clear_ms, 4)
            for form, name in ((0, "direct"), (1, "lds")):
                vo.set_tuning(voxel_form=form)
                fresh, fw, n = timed(lambda: (vm.clear(), fuse(vm)), sync, a.windows)
                warm, ww, _ = timed(lambda: fuse(vm), sync, a.windows)
                case["fuse_%s" % name] = dict(fresh_ms=round(fresh - clear_ms, 4), warm_ms=round(warm, 4), fresh_windows_incl_clear=fw, warm_windows=ww, calls_per_window=n)
            vo.set_tuning(voxel_form=-1)
            fresh, fw, n = timed(lambda: (vm.clear(), insert(vm)), sync, a.windows)
            warm, ww, _ = timed(lambda: insert(vm), sync, a.windows)
            case["insert_points"] = dict(fresh_ms=round(fresh - clear_ms, 4), warm_ms=round(warm, 4), fresh_windows_incl_clear=fw, warm_windows=ww, calls_per_window=n)
            rep_ms, rw, _ = timed(lambda: vo.reproject_dev(p.d_disp.data_ptr(), w, h, B, d_T.data_ptr(), z_min, z_max, 1, d_xyz.data_ptr(), d_valid.data_ptr()), sync, a.windows)
            case["reproject_ms"] = round(rep_ms, 4)
            vm.clear(); fuse(vm)
            st = vm.stats()
            d_out = torch.zeros((st["n_occupied"], 32), dtype=torch.uint8, device=p.dev); d_n = torch.zeros(1, dtype=torch.int64, device=p.dev)
            torch.cuda.synchronize()
            ext_ms, ew, _ = timed(lambda: vo.voxel_extract_dev(vm, -1, 1, d_out.data_ptr(), None, st["n_occupied"], d_n.data_ptr()), sync, a.windows)
            assert int(d_n.cpu()[0]) == st["n_occupied"] and st["n_dropped_full"] == 0 and st["status"] == 0, st
            case["extract_ms"] = round(ext_ms, 4)
            nbytes = 5 * B * h * w
            gbs = vo.hbm_copy_probe(max(nbytes // 2, 1 << 20), 20)   # a copy of nbytes / 2 moves nbytes
            copy_ms = nbytes / gbs * 1e-6
            table_bytes = 32 << log2
            gbs_t = vo.hbm_copy_probe(max(table_bytes // 2, 1 << 20), 20)
            case.update(compulsory_bytes=nbytes, copy_probe_gbs=round(gbs, 1), copy_probe_ms_same_bytes=round(copy_ms, 4),
                        ratio_fuse_direct_fresh=round(case["fuse_direct"]["fresh_ms"] / copy_ms, 2), ratio_fuse_lds_fresh=round(case["fuse_lds"]["fresh_ms"] / copy_ms, 2),
                        ratio_fuse_direct_warm=round(case["fuse_direct"]["warm_ms"] / copy_ms, 2), ratio_fuse_lds_warm=round(case["fuse_lds"]["warm_ms"] / copy_ms, 2),
                        ratio_insert_points_fresh=round(case["insert_points"]["fresh_ms"] / copy_ms, 2),
                        extract_ratio_to_table_read=round(ext_ms / (table_bytes / gbs_t * 1e-6), 2),
                        occupied_voxels=st["n_occupied"], points=st["n_points"], points_per_voxel=round(st["n_points"] / max(st["n_occupied"], 1), 1),
                        dropped_range=st["n_dropped_range"], load_factor=round(st["n_occupied"] / (1 << log2), 3))
            vm.close()
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
        finally:
            p.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
