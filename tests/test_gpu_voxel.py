"""GPU: the dense map stage (include/vslam_hip.h "dense map") -- vslam_reproject_dev against the CPU oracle's find_3d, the voxel table against
the numpy restatement tests/voxel_ref.py bit for bit (keys, counts and every float), the fused kernel (both forms) against reprojection +
insertion, a table that overflows, and every refused argument.  Shapes are small: 131 x 37 images are no multiple of the kernels' 64 x 16 tile
and still span three tiles a row."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import voxel_ref as VR

pytestmark = pytest.mark.gpu
RTOL = 1e-4   # tests/test_gpu_geom.py's tolerance
W, H, B = 131, 37, 3
Z_MIN, Z_MAX = 5.0, 60.0


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t


def _refusals(lib, err, section):
    """no(key, rc): the call returned `err` and left the message tests/golden/refused_messages.json holds under `key` -- the text the library gave
    before its host tier was put in order, which every later library must reproduce"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refused_messages.json")) as f:
        want = json.load(f)[section]

    def no(key, rc):
        assert rc == err, key
        assert lib.vslam_last_error().decode() == want[key], key
    return no


def _poses(synth, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.perturb_pose(synth.se3_from_Rt(np.eye(3), [0.3 * b, -0.1, 2.0 + b]), rng, 0.2) for b in range(n)])


def _same(got, want):
    """two voxel lists equal bit for bit (floats compared as bits)"""
    assert got.dtype == want.dtype and len(got) == len(want), (got.dtype, want.dtype, len(got), len(want))
    for f in got.dtype.names:
        a, b = got[f], want[f]
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert len(bad) == 0, (f, len(bad), got[bad[:3]], want[bad[:3]])


def _reproject(vo, disp, T, step, z_min=Z_MIN, z_max=Z_MAX, d_disp=None):
    """(xyz (B, hs, ws, 3), valid (B, hs, ws)) of vslam_reproject_dev"""
    import torch
    n, h, w = disp.shape
    hs, ws = -(-h // step), -(-w // step)
    d_disp = _dev(disp) if d_disp is None else d_disp
    d_T = _dev(T)
    d_xyz = torch.zeros((n, hs, ws, 3), dtype=torch.float32, device="cuda"); d_valid = torch.full((n, hs, ws), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vo.reproject_dev(d_disp.data_ptr(), w, h, n, d_T.data_ptr(), z_min, z_max, step, d_xyz.data_ptr(), d_valid.data_ptr())
    vo.sync()
    return d_xyz.cpu().numpy(), d_valid.cpu().numpy()


def _random_disparities(seed):
    """B x H x W disparities with the invalid kinds SGBM and a caller can produce, none whose depth lies within 1e-6 relative of a gate"""
    rng = np.random.default_rng(seed)
    disp = rng.uniform(0.5, 90, (B, H, W)).astype(np.float32)
    kind = rng.random((B, H, W))
    disp[kind < 0.10] = -1.0
    disp[(kind >= 0.10) & (kind < 0.13)] = 0.0
    disp[(kind >= 0.13) & (kind < 0.15)] = 1e-6    # a depth far beyond any gate
    disp[(kind >= 0.15) & (kind < 0.17)] = np.nan
    fb = VR_FX * VR_B
    for gate in (Z_MIN, Z_MAX):    # move a disparity off a gate before it is used (none is, at this seed; the assertion below is the check)
        with np.errstate(divide="ignore", invalid="ignore"):
            near = np.abs(fb / disp.astype(np.float64) / gate - 1) <= 1e-5
        disp[near] *= np.float32(1.01)
    return disp


VR_FX, VR_B = 718.856, 0.573


@pytest.mark.parametrize("step", [1, 3])
def test_reproject_matches_oracle_find_3d(vo, oracle, synth, step):
    disp = _random_disparities(3)
    T = _poses(synth, B, 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = VR_FX * VR_B / disp.astype(np.float64)
    fin = np.isfinite(depth)
    for gate in (Z_MIN, Z_MAX):
        assert np.abs(depth[fin] / gate - 1).min() > 1e-6, "a depth on a gate: the valid flags would depend on the last bit"
    xyz, valid = _reproject(vo, disp, T, step)
    rr, cc = np.meshgrid(np.arange(0, H, step), np.arange(0, W, step), indexing="ij")
    assert xyz.shape == (B, rr.shape[0], rr.shape[1], 3)
    kps = np.zeros(rr.size, oracle.KEYPOINT_DTYPE)
    kps["x"] = cc.ravel(); kps["y"] = rr.ravel()
    n_valid = 0
    for b in range(B):
        wx, wv, _ = oracle.find_3d_disparity(kps, disp[b], T[b], depth_gate=(Z_MIN, Z_MAX, Z_MAX))
        gv = valid[b].ravel()
        assert np.array_equal(gv, wv), (b, int((gv != wv).sum()))
        ok = wv.astype(bool)
        assert np.allclose(xyz[b].reshape(-1, 3)[ok], wx[ok], rtol=RTOL, atol=1e-5)
        n_valid += int(ok.sum())
    assert 0.3 * kps.size * B < n_valid < 0.9 * kps.size * B


def _point_lists(voxel_size, seed):
    """clustered points (hundreds per voxel), scattered ones, and a few that are out of range or not finite"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-20, 20, (40, 3))
    clustered = (centres[:, None, :] + rng.normal(0, 0.15 * voxel_size, (40, 300, 3))).reshape(-1, 3)
    scattered = rng.uniform(-30, 30, (3000, 3))
    limit = voxel_size * VR.HALF
    odd = np.array([[limit * 1.5, 0, 0], [0, -limit * 1.5, 0], [0, 0, np.nan], [np.inf, 0, 0], [1e30, 1e30, 1e30], [-1e-12, -1e-12, 1e-12]])
    pts = np.concatenate([clustered, scattered, odd]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return pts, (rng.random(len(pts)) < 0.8).astype(np.uint8), rng.integers(0, 256, len(pts)).astype(np.uint8)


def _insert(vo, vm, pts, valid, inten, map_id):
    d = [_dev(pts), None if valid is None else _dev(valid), None if inten is None else _dev(inten)]
    vo.voxel_insert_points_dev(vm, d[0].data_ptr(), None if d[1] is None else d[1].data_ptr(), None if d[2] is None else d[2].data_ptr(), len(pts), map_id)
    vo.sync()


@pytest.mark.parametrize("voxel_size", [0.2, 0.05])
@pytest.mark.parametrize("with_arrays", [True, False])
def test_insert_and_extract_equal_the_restatement(vo, pkg, voxel_size, with_arrays):
    assert pkg.VOXEL_MAP_DTYPE == VR.VOXEL_MAP_DTYPE
    pa, va, ga = _point_lists(voxel_size, 1)
    pb, vb, gb = _point_lists(voxel_size, 2)
    if not with_arrays:
        va = ga = vb = gb = None
    half = len(pa) // 2
    cut = lambda a, s: None if a is None else a[s]
    ref = VR.VoxelRef(voxel_size)
    ref.insert(pa, va, ga, map_id=0); ref.insert(pb, vb, gb, map_id=VR.MAX_MAP); ref.insert(pb[:500], cut(vb, slice(0, 500)), cut(gb, slice(0, 500)), map_id=0)
    before = vo.device_bytes
    vm, vm2 = vo.voxel_map(voxel_size, 16), vo.voxel_map(voxel_size, 16)
    assert vo.device_bytes - before >= 2 * (32 << 16), "the tables count in vslam_device_bytes"
    try:
        # two inserts in a row ...
        _insert(vo, vm, pa[:half], cut(va, slice(0, half)), cut(ga, slice(0, half)), 0)
        _insert(vo, vm, pa[half:], cut(va, slice(half, None)), cut(ga, slice(half, None)), 0)
        _insert(vo, vm, pb, vb, gb, VR.MAX_MAP)
        _insert(vo, vm, pb[:500], cut(vb, slice(0, 500)), cut(gb, slice(0, 500)), 0)
        # ... equal one insert of both lists
        cat = lambda a, b: None if a is None else np.concatenate([a, b])
        _insert(vo, vm2, np.concatenate([pb[:500], pa]), cat(cut(vb, slice(0, 500)), va), cat(cut(gb, slice(0, 500)), ga), 0)
        _insert(vo, vm2, pb, vb, gb, VR.MAX_MAP)
        want = ref.extract()
        assert want["count"].max() > 100 and (want["count"] == 1).sum() > 1000 and set(want["map"]) == {0, VR.MAX_MAP}
        for m in (vm, vm2):
            _same(m.extract(), want)
            st = m.stats()
            assert st == dict(n_occupied=len(want), n_points=ref.n_points, n_dropped_range=ref.n_dropped_range, n_dropped_full=0, status=0), st
        assert ref.n_dropped_range >= 5 and ref.n_points + ref.n_dropped_range == ref.n_offered
        # the map filter and min_count
        for map_id, min_count in ((0, 1), (VR.MAX_MAP, 1), (7, 1), (-1, 3), (0, 50)):
            _same(vm.extract(map_id=map_id, min_count=min_count), ref.extract(map_id=map_id, min_count=min_count))
        # a capacity below the count: the full count comes back, `capacity` voxels are written, each one of the list
        part = vm.extract(capacity=100)
        assert vm.last_count == len(want) and len(part) == 100
        pos = np.searchsorted(ref.keys, VR.pack_key(part["map"].astype(np.int64), part["ix"].astype(np.int64), part["iy"].astype(np.int64), part["iz"].astype(np.int64)))
        assert len(set(pos.tolist())) == 100
        _same(part, want[pos])
    finally:
        vm.close(); vm2.close()
    assert vo.device_bytes == before


def _plane_disparities():
    """a fronto-parallel plane at 20 m (every pixel of a tile shares a handful of voxels), a nearer band, and invalid pixels"""
    disp = np.full((B, H, W), np.float32(VR_FX * VR_B / 20.0), np.float32)
    disp[:, 20:30, 40:100] = np.float32(VR_FX * VR_B / 8.0)
    disp[:, ::7, ::5] = -1.0
    disp[1] = _random_disparities(8)[1]
    return disp


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("step,with_gray,aligned", [(1, True, True), (1, False, True), (1, True, False), (2, True, True)])
def test_fused_equals_reproject_then_insert(vo, synth, form, step, with_gray, aligned):
    import torch
    disp = _plane_disparities()
    T = _poses(synth, B, 5)
    map_id = np.array([0, -1, 5], np.int32)
    rng = np.random.default_rng(6)
    pitch = 192
    gray = rng.integers(0, 256, (B, H, pitch)).astype(np.uint8)
    # the disparities at a 16-byte aligned address (the kernels' 16-byte row loads) or 4 bytes past one (their pixel-by-pixel loads)
    store = torch.zeros(B * H * W + 1, dtype=torch.float32, device="cuda")
    d_disp = store[:-1] if aligned else store[1:]
    d_disp.copy_(torch.from_numpy(disp.ravel()))
    torch.cuda.synchronize()
    assert (d_disp.data_ptr() % 16 == 0) == aligned
    xyz, valid = _reproject(vo, disp, T, step, d_disp=d_disp)
    two, fused = vo.voxel_map(0.2, 14), vo.voxel_map(0.2, 14)
    ref = VR.VoxelRef(0.2)
    try:
        for b in range(B):
            if map_id[b] < 0:
                continue
            g = np.ascontiguousarray(gray[b, :H:step, :W:step]) if with_gray else None
            _insert(vo, two, xyz[b].reshape(-1, 3), valid[b].ravel(), None if g is None else g.ravel(), int(map_id[b]))
            ref.insert(xyz[b].reshape(-1, 3), valid[b].ravel(), None if g is None else g.ravel(), int(map_id[b]))
        want = two.extract()
        _same(want, ref.extract())
        assert set(want["map"]) == {0, 5} and want["count"].max() > 15, "the plane shares voxels inside a tile"
        d_T, d_id, d_gray = _dev(T), _dev(map_id), _dev(gray)
        vo.set_tuning(voxel_form=form)
        outs = []
        for _ in range(2):   # twice: the same canonical output whatever order the points arrived in
            fused.clear()
            vo.voxel_fuse_disparity_dev(fused, d_disp.data_ptr(), d_gray.data_ptr() if with_gray else None, H * pitch, pitch, W, H, B, d_T.data_ptr(), d_id.data_ptr(),
                                        Z_MIN, Z_MAX, step)
            vo.sync()
            outs.append(fused.extract())
            assert fused.stats() == two.stats()
        _same(outs[0], want); _same(outs[1], want)
    finally:
        vo.set_tuning(voxel_form=-1)
        two.close(); fused.close()


@pytest.mark.parametrize("form", [0, 1])
def test_overflow_drops_points_and_conserves_the_count(vo, synth, form):
    rng = np.random.default_rng(9)
    pts = rng.uniform(-40, 40, (6000, 3)).astype(np.float32)    # ~6000 distinct voxels for 1024 slots
    pts[:10] = np.nan
    disp = _random_disparities(10)
    T = _poses(synth, B, 11)
    _, valid = _reproject(vo, disp, T, 1)
    vm = vo.voxel_map(0.2, 10)
    try:
        _insert(vo, vm, pts, None, None, 3)
        st = vm.stats()
        v = vm.extract()
        assert st["status"] & 1 and st["n_dropped_full"] > 0 and st["n_dropped_range"] == 10
        assert st["n_occupied"] == len(v) <= 1024 and int(v["count"].sum()) == st["n_points"]
        assert st["n_points"] + st["n_dropped_full"] + st["n_dropped_range"] == len(pts)
        # ... and through the fused kernel, on top
        d_disp, d_T, d_id = _dev(disp), _dev(T), _dev(np.zeros(B, np.int32))
        vo.set_tuning(voxel_form=form)
        vo.voxel_fuse_disparity_dev(vm, d_disp.data_ptr(), None, 0, 0, W, H, B, d_T.data_ptr(), d_id.data_ptr(), Z_MIN, Z_MAX, 1)
        st2 = vm.stats()
        v2 = vm.extract()
        assert int(v2["count"].sum()) == st2["n_points"] and st2["n_occupied"] == len(v2) <= 1024
        assert st2["n_points"] + st2["n_dropped_full"] + st2["n_dropped_range"] == len(pts) + int(valid.sum())
        vm.clear()
        assert vm.stats() == dict(n_occupied=0, n_points=0, n_dropped_range=0, n_dropped_full=0, status=0) and len(vm.extract()) == 0
    finally:
        vo.set_tuning(voxel_form=-1)
        vm.close()


def test_refused_arguments(vo, pkg):
    import torch
    lib, ERR = vo.lib, pkg.VSLAM_ERR_ARG
    no = _refusals(lib, ERR, "voxel")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    h = C.c_void_p()
    for size, log2 in ((0.0, 12), (-0.2, 12), (float("nan"), 12), (float("inf"), 12), (1e-60, 12), (0.2, 9), (0.2, 29)):
        no("create %r %d" % (size, log2), lib.vslam_voxel_create(vo.h, size, log2, C.byref(h)))
        assert not h.value, (size, log2)
    no("create null ctx", lib.vslam_voxel_create(None, 0.2, 12, C.byref(h)))
    no("create null out", lib.vslam_voxel_create(vo.h, 0.2, 12, None))
    vm = vo.voxel_map(0.2, 10)
    other = pkg.VO(device=0, max_batch=1)
    try:
        good = dict(d=p, w=16, h=8, B=2, T=p, z0=1.0, z1=50.0, step=1)
        bad = [dict(B=0), dict(B=5), dict(step=0), dict(step=-1), dict(z0=50.0, z1=50.0), dict(z0=60.0), dict(z1=float("nan")), dict(d=None), dict(T=None), dict(w=0), dict(h=0)]
        for kw in bad:
            a = dict(good, **kw)
            head = (a["d"], a["w"], a["h"], a["B"], a["T"], a["z0"], a["z1"], a["step"])
            no("reproject %r" % kw, lib.vslam_reproject_dev(vo.h, *head, p, p))
            no("fuse %r" % kw, lib.vslam_voxel_fuse_disparity_dev(vo.h, vm.h, a["d"], None, 0, 0, a["w"], a["h"], a["B"], a["T"], p, a["z0"], a["z1"], a["step"]))
        head = (p, 16, 8, 2, p, 1.0, 50.0, 1)
        no("reproject null d_xyz", lib.vslam_reproject_dev(vo.h, *head, None, p))
        no("reproject null d_valid", lib.vslam_reproject_dev(vo.h, *head, p, None))
        no("reproject null ctx", lib.vslam_reproject_dev(None, *head, p, p))
        fuse = lambda ctx, m, ids, gray=None, img_bytes=0, pitch=0: lib.vslam_voxel_fuse_disparity_dev(ctx, m, p, gray, img_bytes, pitch, 16, 8, 2, p, ids, 1.0, 50.0, 1)
        no("fuse null d_map_id", fuse(vo.h, vm.h, None))
        no("fuse null map", fuse(vo.h, None, p))
        no("fuse null ctx", fuse(None, vm.h, p))
        no("fuse a map of another context", fuse(other.h, vm.h, p))
        no("fuse pitch below w", fuse(vo.h, vm.h, p, gray=p, img_bytes=16 * 8, pitch=15))
        no("fuse img_bytes below pitch * h", fuse(vo.h, vm.h, p, gray=p, img_bytes=16 * 7, pitch=16))
        for map_id in (-1, 1023, 1 << 20):
            no("insert map_id %d" % map_id, lib.vslam_voxel_insert_points_dev(vo.h, vm.h, p, None, None, 4, map_id))
        no("insert null d_xyz", lib.vslam_voxel_insert_points_dev(vo.h, vm.h, None, None, None, 4, 0))
        no("insert null map", lib.vslam_voxel_insert_points_dev(vo.h, None, p, None, None, 4, 0))
        for map_id in (-2, 1023):
            no("extract map_id %d" % map_id, lib.vslam_voxel_extract_dev(vo.h, vm.h, map_id, 1, p, None, 4, p))
        no("extract null d_n_out", lib.vslam_voxel_extract_dev(vo.h, vm.h, -1, 1, p, None, 4, None))
        no("extract null d_out", lib.vslam_voxel_extract_dev(vo.h, vm.h, -1, 1, None, None, 4, p))
        no("extract null map", lib.vslam_voxel_extract_dev(vo.h, None, -1, 1, p, None, 4, p))
        no("clear null map", lib.vslam_voxel_clear(None))
        no("stats null host", lib.vslam_voxel_stats(vm.h, None))
        no("stats null map", lib.vslam_voxel_stats(None, C.byref(pkg.VoxelStats())))
        st = pkg.VoxelStats(); st.struct_size = 8
        no("stats struct_size", lib.vslam_voxel_stats(vm.h, C.byref(st)))
        no("set_tuning voxel_form 2", lib.vslam_set_tuning(vo.h, b"voxel_form", 2))
        vo.sync()
        assert vm.stats() == dict(n_occupied=0, n_points=0, n_dropped_range=0, n_dropped_full=0, status=0), "a refused call launches nothing"
    finally:
        vm.close(); other.close()
