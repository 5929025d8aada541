"""Micro-benchmark of the surface map's clearance layer, by the method of tools/bench_tsdf.py and on the same inputs: one
KeyframePipeline(depth="sgbm", ba_windows="tracks", anms_num=500) step at each batch size, its disparity maps integrated at voxel 0.2 m, J = 4 over
10 .. 40 m.  At R = 4, 8 and 16 voxels: the sites, the layer's blocks (claimed in the pool, and not), ms per vslam_tsdf_distance_dev call in both
forms, the stage profiler's split of one call into its kernels, the rate of vslam_tsdf_distance_query_dev at 2^20 points, and the library's streaming
copy (vslam_hbm_copy_probe) moving the stage's compulsory bytes -- 8 KiB read per claimed block, 1 KiB written per layer block -- in the same process.

    python tools/bench_tsdf_distance.py [--batches 256,1024] [--radii 4,8,16] [--windows 5] [--out profiles/tsdf_distance.json]

A figure is the median of `--windows` timed windows, each a host clock around enough back-to-back calls to last >= 0.2 s (sized from a pipelined
burst and checked), ending in a synchronise; the profiler is off (it is on for the one call of the kernel split, and of the query kernel, only).
Before anything is timed, the first two frames go into a small map and both forms are compared with the numpy yardstick tests/tsdf_distance_ref.py at R = 8 and R = 16: ids, cell words, counts."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tsdf_distance_ref as DR  # noqa: E402
from stereo_visual_slam_amd.pipeline import KeyframePipeline  # noqa: E402


def timed(call, sync, windows, burst=64):
    """median ms per call over `windows` windows of >= 0.2 s.  The calls here last 15 - 1500 us, of the order of one launch and synchronise, so the
    calls per window come from a pipelined burst of `burst` calls (not from one synchronised call, which would undersize the window); a window
    that still ends early is repeated with more calls"""
    call(); sync()
    t0 = time.perf_counter()
    for _ in range(burst):
        call()
    sync()
    n = max(burst, int(0.22 * burst / max(time.perf_counter() - t0, 1e-6)) + 1)
    wins = []
    while len(wins) < windows:
        sync(); t0 = time.perf_counter()
        for _ in range(n):
            call()
        sync()
        el = time.perf_counter() - t0
        if el < 0.2:
            n = int(n * 0.25 / el) + 1
            continue
        wins.append(el * 1e3 / n)
    return float(np.median(wins)), [round(x, 4) for x in wins], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--radii", default="4,8,16")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--trunc", type=int, default=4)
    ap.add_argument("--z-min", type=float, default=10.0)
    ap.add_argument("--z-max", type=float, default=40.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--unique-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_distance.json"))
    a = ap.parse_args()
    import torch

    import stereo_visual_slam_amd as pkg
    if not torch.cuda.is_available():
        sys.exit("bench_tsdf_distance: no GPU visible (there is nothing to measure without one)")
    res = dict(voxel_size=a.voxel, trunc_voxels=a.trunc, z_min=a.z_min, z_max=a.z_max, windows=a.windows, device=torch.cuda.get_device_name(0), cases=[])
    radii = [int(r) for r in a.radii.split(",")]
    seq = None
    for B in [int(b) for b in a.batches.split(",")]:
        p = KeyframePipeline(B, anms_num=500, unique_frames=a.unique_frames, seed=0, ba_windows="tracks", depth="sgbm", sequence=seq, render_workers=8)
        try:
            seq = p.h_seq
            vo, w, h = p.vo, p.w, p.h
            sync = vo.sync
            p.step()
            T, map_id = p.dense_map_inputs()
            with torch.cuda.stream(p.stream):
                d_T = torch.from_numpy(T).to(p.dev); d_id = torch.from_numpy(map_id).to(p.dev)
            sync()
            integrate = lambda tm, n=B: tm.integrate_dev(p.d_disp.data_ptr(), p.d_imgs.data_ptr(), p.img_bytes, p.pitch, w, h, n, d_T.data_ptr(), d_id.data_ptr(),
                                                         a.z_min, a.z_max, 1)
            # ---- the check: two frames, both forms, against the yardstick
            small = vo.tsdf_map(a.voxel, a.trunc, 14)
            integrate(small, 2)
            ids, vox = small.blocks()
            assert small.stats()["n_dropped_full"] == 0 and len(ids) > 100
            for R in (8, 16):
                log2 = int(64 * len(ids)).bit_length()
                want = DR.layer(ids, vox, -1, 1, R, log2)
                assert not want["void"] and want["counts"][0] > 100
                for form in (0, 1):
                    vo.set_tuning(tsdf_dist_form=form)
                    got = small.distance(radius=R, log2_layer_blocks=log2)
                    assert got["counts"] == want["counts"] and np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["cells"], want["cells"]), \
                        "the layer differs from the yardstick (R %d, form %d)" % (R, form)
            vo.set_tuning(tsdf_dist_form=-1)
            small.close()
            # ---- the map: a pool below half full
            probe = vo.tsdf_map(a.voxel, a.trunc, 19)
            integrate(probe)
            st = probe.stats()
            assert st["n_dropped_full"] == 0, st
            probe.close()
            log2 = max(6, int(2 * st["n_blocks"]).bit_length())
            tm = vo.tsdf_map(a.voxel, a.trunc, log2)
            integrate(tm); sync()
            case = dict(B=B, log2_blocks=log2, blocks=st["n_blocks"], runs=[])
            d_counts = torch.zeros(3, dtype=torch.int64, device=p.dev)
            torch.cuda.synchronize()
            for R in radii:
                dp = pkg.TsdfDistanceParams(struct_size=C.sizeof(pkg.TsdfDistanceParams), map_id=-1, min_weight=1, radius_voxels=R, log2_layer_blocks=log2)
                build = lambda: vo._chk(vo.lib.vslam_tsdf_distance_dev(vo.h, tm.h, C.byref(dp), d_counts.data_ptr()), "vslam_tsdf_distance_dev")
                # the layer's table: the smallest power of two that holds the build's blocks, then twice that (a load factor below one half)
                while True:
                    build(); sync()
                    sites, n_layer, n_b = (int(c) for c in d_counts.cpu().tolist())
                    if n_layer or not st["n_blocks"]:
                        break
                    dp.log2_layer_blocks += 1
                dp.log2_layer_blocks += 1
                run = dict(R=R, log2_layer_blocks=int(dp.log2_layer_blocks), sites=sites, layer_blocks=n_layer, layer_blocks_claimed=n_layer - n_b, layer_blocks_unclaimed=n_b,
                           layer_table_bytes=2257 * (1 << dp.log2_layer_blocks) + 64)
                sums = []
                for form, name in ((0, "form0_masks"), (1, "form1_separable")):
                    vo.set_tuning(tsdf_dist_form=form)
                    build(); sync()
                    assert [int(c) for c in d_counts.cpu().tolist()] == [sites, n_layer, n_b]
                    ms, win, n = timed(build, sync, a.windows)
                    vo.profile_enable(True); vo.profile_read()
                    build(); sync()
                    prof = {k: round(t, 4) for k, (t, _, _) in vo.profile_read().items() if k.startswith("tsdf_dist")}
                    vo.profile_enable(False)
                    d_ids = torch.zeros((max(n_layer, 1), 4), dtype=torch.int32, device=p.dev)
                    d_cells = torch.zeros((max(n_layer, 1), 512), dtype=torch.int16, device=p.dev)
                    d_n = torch.zeros(1, dtype=torch.int64, device=p.dev)
                    torch.cuda.synchronize()
                    vo._chk(vo.lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, d_ids.data_ptr(), d_cells.data_ptr(), n_layer, d_n.data_ptr()), "vslam_tsdf_distance_blocks_dev")
                    sync()
                    assert int(d_n.cpu()[0]) == n_layer
                    sums.append((d_cells.to(torch.int64) & 0xFFFF).sum().item())     # (order-free: the two forms hold the same words)
                    run[name] = dict(ms=round(ms, 4), windows_ms=win, calls_per_window=n, kernels_ms_one_call=prof)
                    if form == 1:   # the query rate, on the layer as it stands
                        lo = d_ids[:, 1:].min(0).values.double() * 8 * a.voxel; hi = (d_ids[:, 1:].max(0).values.double() * 8 + 8) * a.voxel
                        N = 1 << 20
                        with torch.cuda.stream(p.stream):
                            d_xyz = (torch.rand((N, 3), dtype=torch.float64, device=p.dev) * (hi - lo) + lo).contiguous()
                            d_m = torch.zeros(N, dtype=torch.int32, device=p.dev)
                            d_dist = torch.zeros(N, dtype=torch.float32, device=p.dev); d_cls = torch.zeros(N, dtype=torch.uint8, device=p.dev)
                        sync()
                        query = lambda: vo._chk(vo.lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, d_xyz.data_ptr(), d_m.data_ptr(), N, d_dist.data_ptr(), d_cls.data_ptr()),
                                                "vslam_tsdf_distance_query_dev")
                        qms, qwin, qn = timed(query, sync, a.windows)
                        vo.profile_enable(True); vo.profile_read()
                        query(); sync()
                        qprof = {k: round(t, 4) for k, (t, _, _) in vo.profile_read().items() if k.startswith("tsdf_dist")}
                        vo.profile_enable(False)
                        run["query"] = dict(points=N, ms=round(qms, 4), windows_ms=qwin, calls_per_window=qn, points_per_s=round(N / qms * 1e3, 0), kernel_ms_one_profiled_call=qprof,
                                            finite_share=round(float(torch.isfinite(d_dist).double().mean().item()), 4))
                    del d_ids, d_cells
                assert sums[0] == sums[1], "the two forms differ"
                vo.set_tuning(tsdf_dist_form=-1)
                nbytes = 8192 * st["n_blocks"] + 1024 * n_layer
                gbs = vo.hbm_copy_probe(max(nbytes // 2, 1 << 20), 20)   # a copy of nbytes / 2 moves nbytes
                copy_ms = nbytes / gbs * 1e-6
                run.update(compulsory_bytes=nbytes, copy_probe_gbs=round(gbs, 1), copy_probe_ms_same_bytes=round(copy_ms, 4),
                           ratio_form0_over_copy=round(run["form0_masks"]["ms"] / copy_ms, 1), ratio_form1_over_copy=round(run["form1_separable"]["ms"] / copy_ms, 1),
                           ratio_form0_over_form1=round(run["form0_masks"]["ms"] / run["form1_separable"]["ms"], 2))
                case["runs"].append(run)
                print(json.dumps(run), flush=True)
            assert tm.stats()["status"] & ~16 == 0
            tm.close()
            res["cases"].append(case)
            with open(a.out, "w") as f:   # (after every batch size: a run cut short keeps what it measured)
                json.dump(res, f, indent=1)
                f.write("\n")
        finally:
            p.close()


if __name__ == "__main__":
    main()
