"""Micro-benchmark of the surface map stage on the SGBM disparities of the rendered sequence, by the method of tools/bench_voxel.py so that the two
map stages can be read side by side: ms per call of vslam_tsdf_integrate_dev in both integration forms and of vslam_tsdf_extract_dev, the stage
profiler's split of one call into its kernels, and the library's own streaming copy (vslam_hbm_copy_probe) moving the stage's compulsory bytes --
5 B per pixel read, 16 KiB per claimed block for a read and a write -- in the same process; vslam_voxel_fuse_disparity_dev on the same input is
the neighbour figure.

    python tools/bench_tsdf.py [--batches 256,1024] [--voxel 0.2] [--trunc 4] [--z-min 10] [--z-max 40] [--windows 5] [--out profiles/tsdf.json]
                               [--mesh-out profiles/tsdf_mesh.json] [--mesh-only] [--render] [--render-out profiles/tsdf_render.json]

The inputs are one KeyframePipeline(depth="sgbm", ba_windows="tracks", anms_num=500) step at each batch size: its disparity maps, left images and
BA-refined poses (KeyframePipeline.dense_map_inputs).  A figure is the median of `--windows` timed windows, each a host clock around enough
back-to-back calls to last >= 0.2 s, ending in a synchronise; the profiler is off (it is on for the one call of the kernel split only).
"fresh" = into a map cleared before every call (the clear's own time, measured the same way, taken off): every block is claimed; "warm" = into the
map the previous call filled: no block is claimed, every sum is read and written.  Before anything is timed, the first two frames go through both
forms into a small map and are compared with the numpy restatement tests/tsdf_ref.py: the block set, every sum, every surfel.

--mesh-out adds the mesh on the same maps: ms per call of vslam_tsdf_mesh_dev next to vslam_tsdf_extract_dev with the same
arguments, the split of one mesh call into its two kernels, and the copy probe on the mesh's compulsory bytes (8 KiB read per block, 48 + 4 B
written per vertex, 12 B per triangle) and on those plus the vertex-id table's traffic (6 KiB written per block, 12 B read per triangle).  The mesh
of the small map is compared with tests/tsdf_mesh_ref.py before anything is timed.  --mesh-only skips the integration and dense-map figures.

--render measures the ray-cast views on the same maps instead: vslam_tsdf_render_dev for 64 views at the map's first 64 keyframe
poses, at the full image size and at half of it, in both forms, at march 0.5 and 1, over the context's depth range: ms per call, rays/s, evaluated
samples/s, the share of rays that hit, the split of one call into its kernels, and the copy probe on the output bytes (20 B per pixel).  Two views of
the small map at an eighth of the size are compared with tests/tsdf_render_ref.py, in both forms, before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tsdf_mesh_ref as MR  # noqa: E402
import tsdf_ref as TR  # noqa: E402
import tsdf_render_ref as RR  # noqa: E402
from bench_voxel import timed  # noqa: E402
from stereo_visual_slam_amd.pipeline import KeyframePipeline  # noqa: E402


def mesh_case(vo, tm, dev, windows, case):
    """the mesh call and the extract call on the filled map tm (min_weight 2, every map), by the method of the figures above"""
    import torch
    sync = vo.sync
    d_n = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    mesh = lambda v, m, vcap, t, tcap: vo._chk(vo.lib.vslam_tsdf_mesh_dev(vo.h, tm.h, -1, 2, v, m, vcap, t, tcap, d_n.data_ptr()), "vslam_tsdf_mesh_dev")
    mesh(None, None, 0, None, 0); sync()
    nv, nt = (int(c) for c in d_n.cpu().tolist())
    d_v = torch.zeros((max(nv, 1), 48), dtype=torch.uint8, device=dev)
    d_m = torch.zeros(max(nv, 1), dtype=torch.int32, device=dev)
    d_t = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    full = lambda: mesh(d_v.data_ptr(), d_m.data_ptr(), nv, d_t.data_ptr(), nt)
    mesh_ms, mw, n = timed(full, sync, windows)
    count_ms, _, _ = timed(lambda: mesh(None, None, 0, None, 0), sync, windows)
    ext = lambda: vo._chk(vo.lib.vslam_tsdf_extract_dev(vo.h, tm.h, -1, 2, d_v.data_ptr(), d_m.data_ptr(), nv, d_n.data_ptr()), "vslam_tsdf_extract_dev")
    ext_ms, ew, _ = timed(ext, sync, windows)
    full(); sync()
    assert [int(c) for c in d_n.cpu().tolist()] == [nv, nt] and int(d_t.min()) >= 0 and int(d_t.max()) < nv
    vo.profile_enable(True); vo.profile_read()
    full(); sync()
    prof = {k: round(ms, 4) for k, (ms, _, _) in vo.profile_read().items() if k.startswith("tsdf_mesh")}
    vo.profile_enable(False)
    blocks = tm.stats()["n_blocks"]
    compulsory = 8192 * blocks + 52 * nv + 12 * nt
    with_vid = compulsory + 6144 * blocks + 12 * nt
    gbs = vo.hbm_copy_probe(max(compulsory // 2, 1 << 20), 20)
    gbs2 = vo.hbm_copy_probe(max(with_vid // 2, 1 << 20), 20)
    case.update(vertices_min_weight_2=nv, triangles_min_weight_2=nt, mesh_ms=round(mesh_ms, 4), mesh_windows=mw, calls_per_window=n, mesh_count_only_ms=round(count_ms, 4),
                extract_ms=round(ext_ms, 4), extract_windows=ew, ratio_mesh_over_extract=round(mesh_ms / ext_ms, 2), kernels_ms_one_call=prof,
                compulsory_bytes=compulsory, copy_probe_gbs=round(gbs, 1), copy_probe_ms_compulsory=round(compulsory / gbs * 1e-6, 4),
                bytes_with_vertex_ids=with_vid, copy_probe_ms_with_vertex_ids=round(with_vid / gbs2 * 1e-6, 4),
                ratio_mesh_over_copy=round(mesh_ms / (compulsory / gbs * 1e-6), 2))
    return case


def render_case(vo, pkg, tm, dev, windows, T, map_id, w, h, case):
    """vslam_tsdf_render_dev on the filled map tm: V views at the poses T, two sizes x two forms x two marches, by the method of the figures above"""
    import ctypes as C

    import torch
    sync = vo.sync
    V = len(T)
    p = vo.params
    d_T = torch.from_numpy(np.ascontiguousarray(T)).to(dev); d_id = torch.from_numpy(np.ascontiguousarray(map_id, np.int32)).to(dev)
    d_counts = torch.zeros(2, dtype=torch.int64, device=dev)
    case.update(views=V, z_min=float(p.depth_min), z_max=float(p.depth_reliable), runs=[])
    for scale in (1.0, 0.5):
        ws, hs = int(round(w * scale)), int(round(h * scale))
        d_depth = torch.zeros((V, hs, ws), dtype=torch.float32, device=dev)
        d_attr = torch.zeros((V, hs, ws, 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        out_bytes = 20 * V * hs * ws
        gbs = vo.hbm_copy_probe(max(out_bytes // 2, 1 << 20), 20)   # a copy of out_bytes / 2 moves out_bytes
        for march in (0.5, 1.0):
            rp = pkg.TsdfRenderParams(w=ws, h=hs, fx=p.cam[0] * scale, fy=p.cam[1] * scale, cx=p.cam[2] * scale, cy=p.cam[3] * scale, z_min=p.depth_min,
                                      z_max=p.depth_reliable, march=march, min_weight=1)
            call = lambda counts=None: vo.tsdf_render_dev(tm, rp, V, d_T.data_ptr(), d_id.data_ptr(), d_depth.data_ptr(), d_attr.data_ptr(), counts)
            kept = None
            for form in (0, 1):
                vo.set_tuning(tsdf_render_form=form)
                call(d_counts.data_ptr()); sync()
                hits, samples = (int(c) for c in d_counts.cpu().tolist())
                bits = (d_depth.view(torch.int32).sum(dtype=torch.int64).item(), d_attr.view(torch.int32).sum(dtype=torch.int64).item())
                assert kept is None or kept == (hits, bits), "the two forms differ"
                kept = (hits, bits)
                ms, win, n = timed(call, sync, windows)
                vo.profile_enable(True); vo.profile_read()
                call(); sync()
                prof = {k: round(t, 4) for k, (t, _, _) in vo.profile_read().items() if k.startswith("tsdf_")}
                vo.profile_enable(False)
                rays = V * hs * ws
                run = dict(w=ws, h=hs, march=march, form=form, ms=round(ms, 4), windows_ms=win, calls_per_window=n, rays=rays, rays_per_s=round(rays / ms * 1e3, 0),
                           samples=samples, samples_per_s=round(samples / ms * 1e3, 0), samples_per_ray=round(samples / rays, 2), hit_share=round(hits / rays, 4),
                           kernels_ms_one_call=prof, output_bytes=out_bytes, copy_probe_gbs=round(gbs, 1), copy_probe_ms_output_bytes=round(out_bytes / gbs * 1e-6, 4),
                           ratio_over_copy=round(ms / (out_bytes / gbs * 1e-6), 1))
                case["runs"].append(run)
                print(json.dumps(run), flush=True)
            vo.set_tuning(tsdf_render_form=-1)
        del d_depth, d_attr
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--trunc", type=int, default=4)
    ap.add_argument("--z-min", type=float, default=10.0)
    ap.add_argument("--z-max", type=float, default=40.0)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--unique-frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mesh-out", default=None)
    ap.add_argument("--mesh-only", action="store_true")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--render-out", default=os.path.join(ROOT, "profiles", "tsdf_render.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tsdf: no GPU visible (there is nothing to measure without one)")
    res = dict(voxel_size=a.voxel, trunc_voxels=a.trunc, z_min=a.z_min, z_max=a.z_max, windows=a.windows, device=torch.cuda.get_device_name(0), cases=[])
    mres = dict(res, cases=[])
    rres = dict(res, cases=[])
    seq = None
    for B in [int(b) for b in a.batches.split(",")]:
        p = KeyframePipeline(B, anms_num=500, unique_frames=a.unique_frames, seed=0, ba_windows="tracks", depth="sgbm", sequence=seq, render_workers=8)
        try:
            seq = p.h_seq
            vo, w, h = p.vo, p.w, p.h
            p.step()
            T, map_id = p.dense_map_inputs()
            with torch.cuda.stream(p.stream):
                d_T = torch.from_numpy(T).to(p.dev); d_id = torch.from_numpy(map_id).to(p.dev)
            vo.sync()
            integrate = lambda tm, n=B: tm.integrate_dev(p.d_disp.data_ptr(), p.d_imgs.data_ptr(), p.img_bytes, p.pitch, w, h, n, d_T.data_ptr(), d_id.data_ptr(),
                                                         a.z_min, a.z_max, 1)
            # ---- the check: two frames, both forms, against the restatement
            assert (map_id[:2] == 0).all()
            ref = TR.TsdfRef(a.voxel, a.trunc, list(vo.params.cam))
            ref.integrate(p.d_disp[:2].cpu().numpy(), np.ascontiguousarray(p.h_imgs[:2]), T[:2], map_id[:2], a.z_min, a.z_max)
            want_ids, want_vox = ref.dump()
            want = ref.extract()
            small = vo.tsdf_map(a.voxel, a.trunc, max(8, int(2 * len(want_ids)).bit_length()))
            for form in (0, 1):
                vo.set_tuning(tsdf_form=form)
                small.clear(); integrate(small, 2)
                ids, vox = small.blocks()
                assert np.array_equal(ids, want_ids) and np.array_equal(vox, want_vox) and small.stats()["n_dropped_full"] == 0, "the surface map differs from the restatement (form %d)" % form
                assert small.extract().tobytes() == want.tobytes(), "the surfels differ from the restatement (form %d)" % form
            if a.mesh_out:
                for mw in (1, 2):
                    gv, gt = small.mesh(min_weight=mw)
                    wv, wt = MR.mesh(want_ids, want_vox, a.voxel, mw)
                    assert gv.tobytes() == wv.tobytes() and np.array_equal(gt, wt) and len(wt) > 0, "the mesh differs from the yardstick (min_weight %d)" % mw
            if a.render:   # two views of the small map at an eighth of the size, both forms, against the yardstick
                import stereo_visual_slam_amd as pkg
                K4, size = tuple(float(v) / 8 for v in vo.params.cam[:4]), (w // 8, h // 8)
                rwant = RR.render(want_ids, want_vox, a.voxel, T[:2], map_id[:2], K4, size, a.z_min / 2, a.z_max, 0.5, 1)
                assert rwant["hits"] > 100, rwant["hits"]
                for form in (0, 1):
                    vo.set_tuning(tsdf_render_form=form)
                    got = small.render(T[:2], map_id[:2], K4=K4, size=size, z_min=a.z_min / 2, z_max=a.z_max)
                    gattr = np.concatenate([got["normal"], got["intensity"][..., None]], -1)
                    assert got["depth"].tobytes() == rwant["depth"].tobytes() and gattr.tobytes() == rwant["attr"].tobytes() and got["counts"][0] == rwant["hits"], \
                        "the views differ from the yardstick (form %d)" % form
                vo.set_tuning(tsdf_render_form=-1)
            small.close()
            # ---- the pool: a load factor below one half
            probe = vo.tsdf_map(a.voxel, a.trunc, 19)
            integrate(probe)
            st = probe.stats()
            assert st["n_dropped_full"] == 0, st
            probe.close()
            log2 = max(6, int(2 * st["n_blocks"]).bit_length())
            tm = vo.tsdf_map(a.voxel, a.trunc, log2)
            sync = vo.sync
            case = dict(B=B, log2_blocks=log2, pixels=B * h * w, blocks=st["n_blocks"], alloc_samples=st["n_samples"], dropped_range=st["n_dropped_range"],
                        load_factor=round(st["n_blocks"] / (1 << log2), 3))
            if a.mesh_out:
                integrate(tm); sync()
                mcase = mesh_case(vo, tm, p.dev, a.windows, dict(case))
                mres["cases"].append(mcase)
                print(json.dumps(mcase), flush=True)
                with open(a.mesh_out, "w") as f:
                    json.dump(mres, f, indent=1)
                    f.write("\n")
                tm.clear(); sync()
            if a.render:
                integrate(tm); sync()
                rcase = render_case(vo, pkg, tm, p.dev, a.windows, T[:64], map_id[:64], w, h, dict(case))
                rres["cases"].append(rcase)
                with open(a.render_out, "w") as f:
                    json.dump(rres, f, indent=1)
                    f.write("\n")
            if a.mesh_only or a.render:
                tm.close()
                continue
            clear_ms, _, _ = timed(tm.clear, sync, a.windows)
            case["clear_ms"] = round(clear_ms, 4)
            for form, name in ((0, "walk_all"), (1, "masks")):
                vo.set_tuning(tsdf_form=form)
                fresh, fw, n = timed(lambda: (tm.clear(), integrate(tm)), sync, a.windows)
                warm, ww, _ = timed(lambda: integrate(tm), sync, a.windows)
                # the kernel split of one fresh call, the stage profiler on for this call only
                tm.clear(); sync()
                vo.profile_enable(True); vo.profile_read()
                integrate(tm); sync()
                prof = {k: round(ms, 4) for k, (ms, _, _) in vo.profile_read().items() if k.startswith("tsdf_")}
                vo.profile_enable(False)
                s = tm.stats()
                case["integrate_%s" % name] = dict(fresh_ms=round(fresh - clear_ms, 4), warm_ms=round(warm, 4), fresh_windows_incl_clear=fw, warm_windows=ww,
                                                   calls_per_window=n, kernels_ms_one_fresh_call=prof, pairs_visited=s["n_pairs_visited"], pairs_kept=s["n_pairs_kept"],
                                                   voxel_samples_per_s=round(s["n_pairs_kept"] * 512 / max(prof.get("tsdf_integrate_kernel", 0.0), 1e-9) * 1e3, 0))
            vo.set_tuning(tsdf_form=-1)
            tm.clear(); integrate(tm)
            st = tm.stats()
            d_n = torch.zeros(1, dtype=torch.int64, device=p.dev)
            torch.cuda.synchronize()
            vo._chk(vo.lib.vslam_tsdf_extract_dev(vo.h, tm.h, -1, 2, None, None, 0, d_n.data_ptr()), "vslam_tsdf_extract_dev"); sync()
            n_surf = int(d_n.cpu()[0])
            d_out = torch.zeros((max(n_surf, 1), 48), dtype=torch.uint8, device=p.dev)
            torch.cuda.synchronize()
            ext_ms, ew, _ = timed(lambda: vo._chk(vo.lib.vslam_tsdf_extract_dev(vo.h, tm.h, -1, 2, d_out.data_ptr(), None, n_surf, d_n.data_ptr()), "vslam_tsdf_extract_dev"),
                                  sync, a.windows)
            assert int(d_n.cpu()[0]) == n_surf and st["n_dropped_full"] == 0 and tm.stats()["status"] == 0, st
            case.update(extract_ms=round(ext_ms, 4), surfels_min_weight_2=n_surf)
            tm.close()
            # ---- the neighbour: the dense map's fused pass on the same input (its default form, a table below half full)
            vprobe = vo.voxel_map(a.voxel, 26)
            fuse = lambda vm: vo.voxel_fuse_disparity_dev(vm, p.d_disp.data_ptr(), p.d_imgs.data_ptr(), p.img_bytes, p.pitch, w, h, B, d_T.data_ptr(), d_id.data_ptr(),
                                                          a.z_min, a.z_max, 1)
            fuse(vprobe)
            occ = vprobe.stats()["n_occupied"]
            vprobe.close()
            vm = vo.voxel_map(a.voxel, max(10, int(2 * occ).bit_length()))
            vclear, _, _ = timed(vm.clear, sync, a.windows)
            vfresh, _, _ = timed(lambda: (vm.clear(), fuse(vm)), sync, a.windows)
            vm.close()
            case.update(voxel_fuse_fresh_ms=round(vfresh - vclear, 4), voxel_occupied=occ)
            # ---- the compulsory bytes through the library's streaming copy
            nbytes = 5 * B * h * w + (16 << 10) * st["n_blocks"]
            gbs = vo.hbm_copy_probe(max(nbytes // 2, 1 << 20), 20)   # a copy of nbytes / 2 moves nbytes
            copy_ms = nbytes / gbs * 1e-6
            case.update(compulsory_bytes=nbytes, copy_probe_gbs=round(gbs, 1), copy_probe_ms_same_bytes=round(copy_ms, 4),
                        ratio_walk_all_fresh=round(case["integrate_walk_all"]["fresh_ms"] / copy_ms, 2), ratio_masks_fresh=round(case["integrate_masks"]["fresh_ms"] / copy_ms, 2))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            if a.out:   # (after every batch size: a run cut short keeps what it measured)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")
        finally:
            p.close()


if __name__ == "__main__":
    main()
