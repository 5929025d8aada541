"""GPU: the surface map's ray-cast views (vslam_tsdf_render_dev) against the numpy yardstick tests/tsdf_render_ref.py over the fields of
tests/tsdf_mesh_cases.py: depth and attributes compared as bits, in both forms (tuning key tsdf_render_form); the hit count; views that take no
part; image sizes off the tile; canaries behind both outputs; a NULL attribute buffer; the bounds of form 1's tile ranges; a full pool; repeated
calls; every refused argument.  The largest field is 27 blocks, the largest call three views of 67 x 45."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_render_cases as RC
import tsdf_render_ref as RR

pytestmark = pytest.mark.gpu
FORMS = [0, 1]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """a TsdfMap.render() result against the yardstick's, bit for bit"""
    attr = np.concatenate([got["normal"], got["intensity"][..., None]], -1)
    for name, g, w in (("depth", got["depth"], want["depth"]), ("attr", attr, want["attr"])):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.argwhere(_bits(g) != _bits(w))
        assert len(bad) == 0, (name, len(bad), bad[:3].tolist(), [g[tuple(b)] for b in bad[:3]], [w[tuple(b)] for b in bad[:3]])
    assert got["counts"][0] == want["hits"], (got["counts"], want["hits"])


def _render(vo, tm, form, want=None, **kw):
    """tm.render in one form with the arguments the yardstick's result `want` was made with (overridden by kw)"""
    a = {} if want is None else dict(T_c_w=want["T"], map_id=want["map_id"], K4=want["cam"], size=want["size"], z_min=want["z_min"], z_max=want["z_max"],
                                     march=want["march"], min_weight=want["min_weight"])
    a.update(kw)
    vo.set_tuning(tsdf_render_form=form)
    try:
        return tm.render(**a)
    finally:
        vo.set_tuning(tsdf_render_form=-1)


def _loaded(vo, ids, voxels, voxel_size, log2_blocks=8):
    tm = vo.tsdf_map(voxel_size, 3, log2_blocks)
    tm.load_blocks(ids, voxels)
    return tm


@pytest.fixture(scope="module")
def maps(vo):
    """every case loaded once into a map of its own"""
    made = {}
    for name in ("noise_full", "noise_holes", "two_maps", "sphere"):
        c = MC.cases()[name]
        made[name] = _loaded(vo, c["ids"], c["voxels"], c["voxel_size"])
    yield made
    for tm in made.values():
        tm.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("march", [1.0, 0.5, 0.25])
def test_sphere(vo, maps, march, form):
    want = RC.reference_of("sphere", march)
    assert want["hits"] > 3000
    _same(_render(vo, maps["sphere"], form, want), want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("min_weight", [1, 2])
@pytest.mark.parametrize("name", ["noise_full", "noise_holes"])
def test_noise_from_outside_and_from_inside_and_again(vo, maps, name, min_weight, form):
    """exact zeros, absent blocks, weights at 2^20, sign changes everywhere; 67 x 45 is no multiple of the tile; the third camera sits inside the
    field (form 1: inside a claimed block of noise_full, with blocks behind it); a second call gives the same bytes"""
    want = RC.reference_of(name, 0.5, min_weight)
    assert want["hits"] > 100, want["hits"]
    got = _render(vo, maps[name], form, want)
    _same(got, want)
    again = _render(vo, maps[name], form, want)
    assert all(got[k].tobytes() == again[k].tobytes() for k in ("depth", "normal", "intensity")) and got["counts"] == again["counts"]


@pytest.mark.parametrize("form", FORMS)
def test_two_maps_and_views_that_take_no_part(vo, maps, form):
    want = RC.reference_of("two_maps")
    assert (want["depth"][0] > 0).sum() > 100 and (want["depth"][1] > 0).sum() > 100
    got = _render(vo, maps["two_maps"], form, want)
    _same(got, want)
    for k in ("depth", "normal", "intensity"):   # a map without blocks, map id -1, a NaN pose
        assert not _bits(got[k][2:]).any(), k


@pytest.mark.parametrize("form", FORMS)
def test_a_scene_integrated_on_the_device_then_rendered(pkg, form):
    import torch
    case = TC.cases()["scene"]
    want = RC.reference_of("scene")
    vo = pkg.VO(device=0, max_batch=8, cam=case["cam"], img_w=case["disp"].shape[2], img_h=case["disp"].shape[1])
    try:
        empty = vo.device_bytes
        tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
        n, h, w = case["disp"].shape
        pitch = case["gray"].shape[2]
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (case["disp"], case["gray"], case["T"], case["map_id"])]
        torch.cuda.synchronize()
        tm.integrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, n, d[2].data_ptr(), d[3].data_ptr(), case["z_min"], case["z_max"], case["step"])
        vo.sync()
        before = vo.device_bytes
        # camera and size default to the context's: the scene's own
        got = _render(vo, tm, form, T_c_w=case["T"], map_id=case["map_id"], z_min=case["z_min"], z_max=case["z_max"])
        _same(got, want)
        # the view table (and form 1's range table) is the map's, counted while the map lives
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        assert vo.device_bytes - before == n * 128 + (n * tiles * 8 if form == 1 else 0)
        tm.close()
        assert vo.device_bytes == empty
    finally:
        vo.close()


@pytest.mark.parametrize("form", FORMS)
def test_one_pixel_and_no_views(vo, maps, form):
    c = MC.cases()["noise_full"]
    T = RC.noise_views()[:2]
    z0, z1 = RC.NOISE_Z
    want = RR.render(c["ids"], c["voxels"], c["voxel_size"], T, [0, 0], (40.0, 40.0, 3.2, -1.9), (1, 1), z0, z1, 0.5)
    want.update(T=T, map_id=[0, 0], cam=(40.0, 40.0, 3.2, -1.9), size=(1, 1), z_min=z0, z_max=z1, march=0.5, min_weight=1)
    assert want["hits"] >= 1
    _same(_render(vo, maps["noise_full"], form, want), want)
    got = _render(vo, maps["noise_full"], form, want, T_c_w=np.zeros((0, 7)), map_id=np.zeros(0, np.int32))
    assert got["depth"].shape == (0, 1, 1) and got["counts"] == (0, 0)


def _params(pkg, want, **kw):
    fx, fy, cx, cy = want["cam"]
    a = dict(w=want["size"][0], h=want["size"][1], fx=fx, fy=fy, cx=cx, cy=cy, z_min=want["z_min"], z_max=want["z_max"], march=want["march"], min_weight=want["min_weight"])
    a.update(kw)
    rp = pkg.TsdfRenderParams(**a)
    rp.struct_size = C.sizeof(pkg.TsdfRenderParams)
    return rp


@pytest.mark.parametrize("form", FORMS)
def test_canaries_behind_both_outputs_and_a_null_attribute_buffer(vo, pkg, maps, form):
    import torch
    want = RC.reference_of("noise_holes")
    V, (w, h) = len(want["T"]), want["size"]
    n, extra = V * h * w, 256
    d_T = torch.from_numpy(np.ascontiguousarray(want["T"])).to("cuda")
    d_id = torch.from_numpy(np.ascontiguousarray(want["map_id"], np.int32)).to("cuda")
    d_depth = torch.full((n + extra,), -77.0, dtype=torch.float32, device="cuda")
    d_attr = torch.full((4 * n + extra,), -77.0, dtype=torch.float32, device="cuda")
    d_depth2 = torch.full((n + extra,), -77.0, dtype=torch.float32, device="cuda")
    d_counts = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vo.set_tuning(tsdf_render_form=form)
    try:
        rp = _params(pkg, want)
        vo.tsdf_render_dev(maps["noise_holes"], rp, V, d_T.data_ptr(), d_id.data_ptr(), d_depth.data_ptr(), d_attr.data_ptr(), d_counts.data_ptr())
        vo.tsdf_render_dev(maps["noise_holes"], rp, V, d_T.data_ptr(), d_id.data_ptr(), d_depth2.data_ptr(), None, None)
        vo.sync()
    finally:
        vo.set_tuning(tsdf_render_form=-1)
    depth, attr, depth2 = d_depth.cpu().numpy(), d_attr.cpu().numpy(), d_depth2.cpu().numpy()
    assert (depth[n:] == -77.0).all() and (attr[4 * n:] == -77.0).all() and (depth2[n:] == -77.0).all()
    assert np.array_equal(_bits(depth[:n]), _bits(want["depth"]).ravel()) and np.array_equal(_bits(attr[:4 * n]), _bits(want["attr"]).ravel())
    assert depth2.tobytes() == depth.tobytes(), "the depth does not depend on the attribute buffer"
    counts = d_counts.cpu().tolist()
    assert counts[0] == want["hits"] and counts[1] >= want["hits"]


@pytest.mark.parametrize("form", FORMS)
def test_blocks_cut_by_z_min_and_beyond_z_max(vo, maps, form):
    """the first camera is 5.3 m from the field's centre and the field 4.8 m wide: the range 4.5 .. 6 m starts and ends inside it"""
    c = MC.cases()["noise_full"]
    T = RC.noise_views()[:1]
    want = RR.render(c["ids"], c["voxels"], c["voxel_size"], T, [0], RC.NOISE_CAM, RC.NOISE_SIZE, 4.5, 6.0, 0.5)
    want.update(T=T, map_id=[0], cam=RC.NOISE_CAM, size=RC.NOISE_SIZE, z_min=4.5, z_max=6.0, march=0.5, min_weight=1)
    full = RC.reference_of("noise_full")
    assert want["hits"] > 200 and (_bits(want["depth"][0]) != _bits(full["depth"][0])).sum() > 200, "the gates change the view"
    _same(_render(vo, maps["noise_full"], form, want), want)


@pytest.mark.parametrize("form", FORMS)
def test_a_quaternion_that_is_not_unit(vo, maps, form):
    """the rule takes the rotation matrix as se3::rotmat forms it, orthonormal or not; form 1's projection needs it orthonormal and gives such a
    view the whole march instead"""
    c = MC.cases()["noise_full"]
    T = RC.noise_views()[:2].copy()
    T[:, :4] *= np.array([[1.02], [0.97]])
    cam, size = RC.NOISE_CAM, (35, 23)
    want = RR.render(c["ids"], c["voxels"], c["voxel_size"], T, [0, 0], cam, size, *RC.NOISE_Z, 0.5)
    want.update(T=T, map_id=[0, 0], cam=cam, size=size, z_min=RC.NOISE_Z[0], z_max=RC.NOISE_Z[1], march=0.5, min_weight=1)
    assert want["hits"] > 100, want["hits"]
    _same(_render(vo, maps["noise_full"], form, want), want)


@pytest.mark.parametrize("form", FORMS)
def test_blocks_at_the_last_block_coordinates(vo, form):
    """block coordinates 2^14 - 1 and -2^14: a sample whose corner index would reach 2^17 is unknown (i + 1 < 2^17), one at -2^17 is not"""
    c = MC.cases()["noise_full"]
    top, low = (1 << 14) - 1, -(1 << 14)
    ids = np.array([[0, top, top, top], [0, low, low, low]], np.int32)
    vox = c["voxels"][:2]
    vs = 0.2
    ctr = lambda b: (8 * b + 4.0) * np.float64(np.float32(vs))
    T = np.stack([RR.look_at((ctr(top) - 2.0, ctr(top) - 0.4, ctr(top) - 0.3), (ctr(top),) * 3), RR.look_at((ctr(top) + 2.1, ctr(top) + 0.3, ctr(top) + 0.5), (ctr(top),) * 3),
                  RR.look_at((ctr(low) - 2.0, ctr(low) - 0.4, ctr(low) - 0.3), (ctr(low),) * 3), RR.look_at((ctr(low) + 2.1, ctr(low) + 0.3, ctr(low) + 0.5), (ctr(low),) * 3)])
    cam, size = (60.0, 60.0, 16.3, 12.7), (33, 25)
    want = RR.render(ids, vox, vs, T, [0] * 4, cam, size, 0.25, 5.0, 0.5)
    want.update(T=T, map_id=[0] * 4, cam=cam, size=size, z_min=0.25, z_max=5.0, march=0.5, min_weight=1)
    assert all((want["depth"][v] > 0).sum() > 20 for v in range(4)), [(want["depth"][v] > 0).sum() for v in range(4)]
    tm = _loaded(vo, ids, vox, vs, 6)
    try:
        assert tm.stats()["n_blocks"] == 2
        _same(_render(vo, tm, form, want), want)
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_a_full_pool(vo, form):
    """100 blocks offered to 64 slots: the render of what blocks() says is held equals the yardstick's of those blocks (lookups of the absent ones end
    at the probe limit)"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-2, 2), indexing="ij"), -1).reshape(-1, 3)
    ids = np.concatenate([np.zeros((100, 1), np.int32), g.astype(np.int32)], 1)
    W, q, Wc, I = MC._field(rng, 100, 1, 3)
    tm = vo.tsdf_map(0.2, 3, 6)
    try:
        tm.load_blocks(ids, MC._voxels(W, q, Wc, I))
        st = tm.stats()
        held_ids, held_vox = tm.blocks()
        assert st["n_blocks"] == len(held_ids) == 64 and st["n_dropped_full"] == 36, st
        T = np.stack([RR.look_at((-7.1, 0.9, 0.7), (0.8, 0.8, 0.0)), RR.look_at((0.73, 0.85, 0.1), (3.0, 1.4, 2.0))])
        cam, size = (30.0, 30.0, 23.4, 15.6), (47, 31)
        want = RR.render(held_ids, held_vox, 0.2, T, [0, 0], cam, size, 0.25, 12.0, 0.5)
        want.update(T=T, map_id=[0, 0], cam=cam, size=size, z_min=0.25, z_max=12.0, march=0.5, min_weight=1)
        assert want["hits"] > 200, want["hits"]
        _same(_render(vo, tm, form, want), want)
    finally:
        tm.close()


def test_refused_arguments(vo, pkg, maps):
    import torch
    lib, ERR = vo.lib, pkg.VSLAM_ERR_ARG
    want = RC.reference_of("noise_holes")
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    tm = maps["noise_holes"]
    other = pkg.VO(device=0, max_batch=1)
    nan, inf = float("nan"), float("inf")
    try:
        def call(ctx=vo.h, m=tm.h, V=1, T=p, ids=p, depth=p, attr=p, counts=p, size=None, null_params=False, **kw):
            rp = _params(pkg, want, **kw)
            if size is not None:
                rp.struct_size = size
            return lib.vslam_tsdf_render_dev(ctx, m, None if null_params else C.byref(rp), V, T, ids, depth, attr, counts)
        assert call(m=None) == ERR and call(ctx=None) == ERR and call(ctx=other.h) == ERR, "a null map, a map of another context"
        assert call(size=0) == ERR and call(size=C.sizeof(pkg.TsdfRenderParams) + 8) == ERR and call(null_params=True) == ERR
        assert call(w=0) == ERR and call(h=0) == ERR and call(w=-3) == ERR and call(V=-1) == ERR
        assert call(V=1 << 15, w=256, h=256) == ERR and call(V=1, w=1 << 16, h=1 << 15) == ERR, "V * h * w at 2^31"
        for k in ("fx", "fy"):
            assert call(**{k: 0.0}) == ERR and call(**{k: -1.0}) == ERR and call(**{k: nan}) == ERR and call(**{k: inf}) == ERR, k
        for k in ("cx", "cy"):
            assert call(**{k: nan}) == ERR and call(**{k: inf}) == ERR, k
        assert call(z_min=0.0) == ERR and call(z_min=-1.0) == ERR and call(z_min=nan) == ERR and call(z_min=inf) == ERR
        assert call(z_max=want["z_min"]) == ERR and call(z_max=0.1) == ERR and call(z_max=nan) == ERR and call(z_max=inf) == ERR
        assert call(march=0.1249) == ERR and call(march=1.0001) == ERR and call(march=nan) == ERR and call(march=0.0) == ERR and call(march=-0.5) == ERR
        assert call(z_min=1.0, z_max=1.0 + 8193 * 0.125 * np.float64(np.float32(0.2)), march=0.125) == ERR, "K above 8192"
        assert call(T=None) == ERR and call(ids=None) == ERR and call(depth=None) == ERR
        assert call(attr=p + 8) == ERR and call(counts=p + 4) == ERR, "alignment"
        assert lib.vslam_last_error().decode().startswith("vslam_tsdf_render_dev")
        vo.sync()
        assert not buf.cpu().numpy().any(), "a refused call launches nothing"
        # what is allowed: no views (with null buffers), no attributes, no counts, a min_weight below 1, march at both ends, K at 8192
        assert call(V=0, T=None, ids=None, depth=None, attr=None, counts=None) == 0
        assert call(attr=None, counts=None) == 0 and call(min_weight=-5) == 0 and call(march=0.125) == 0 and call(march=1.0) == 0
        assert call(z_min=1.0, z_max=1.0 + 8192 * 0.125 * np.float64(np.float32(0.2)), march=0.125, w=4, h=4) == 0
        vo.sync()
    finally:
        other.close()
