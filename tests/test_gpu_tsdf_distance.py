"""GPU: the surface map's clearance layer (include/vslam_hip.h "DISTANCE") against the numpy yardstick tests/tsdf_distance_ref.py, bit for bit: the
layer's blocks and cell words, the three counts, the status and 4096 point queries, over every case of tests/tsdf_distance_cases.py in both forms;
a layer built twice; a capacity below the count; staleness after every call that changes the map; the bytes the handle holds; every refusal.
Hand-made fields go in through TsdfMap.load_blocks; the two scenes of tests/tsdf_cases.py are integrated (160 x 48 and 37 x 48, at most four frames)."""
import ctypes as C

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_distance_cases as DC
import tsdf_distance_ref as DR

pytestmark = pytest.mark.gpu
FORMS = [0, 1]
STALE = "distance layer not built or older than the map"


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def vos(pkg):
    """one context per camera (the integration reads the camera from the context; hand-made fields use the first scene's)"""
    made = {}

    def get(scene="scene"):
        case = TC.cases()[scene]
        key = (case["cam"], case["disp"].shape[2])
        if key not in made:
            made[key] = pkg.VO(device=0, max_batch=8, cam=case["cam"], img_w=case["disp"].shape[2], img_h=case["disp"].shape[1])
        return made[key]

    yield get
    for v in made.values():
        v.close()


def _integrate(vo, tm, case, frames):
    fr = list(frames)
    disp, gray = case["disp"][fr], case["gray"][fr]
    n, h, w = disp.shape
    pitch = gray.shape[2]
    d = [_dev(disp), _dev(gray), _dev(case["T"][fr]), _dev(case["map_id"][fr])]
    tm.integrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, n, d[2].data_ptr(), d[3].data_ptr(), case["z_min"], case["z_max"], case["step"])
    vo.sync()


def _map_of(vos, name):
    """(vo, a TsdfMap that holds the case's field, its voxel size)"""
    c = DC.cases()[name]
    if c["scene"] is None:
        vo = vos()
        tm = vo.tsdf_map(c["voxel_size"], 4, DC.LOG2_POOL)
        tm.load_blocks(c["ids"], c["vox"])
        return vo, tm, c["voxel_size"]
    case = TC.cases()[c["scene"]]
    vo = vos(c["scene"])
    tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
    _integrate(vo, tm, case, range(len(case["disp"])))
    return vo, tm, case["voxel_size"]


def _build(vo, tm, b, form):
    vo.set_tuning(tsdf_dist_form=form)
    try:
        return tm.distance(map_id=b["map_id"], min_weight=b["min_weight"], radius=b["radius"], log2_layer_blocks=b["log2"])
    finally:
        vo.set_tuning(tsdf_dist_form=-1)


def _same_layer(got, want):
    assert tuple(got["counts"]) == tuple(want["counts"]), (got["counts"], want["counts"])
    assert got["ids"].dtype == np.int32 and got["cells"].dtype == np.uint16
    assert got["ids"].shape == want["ids"].shape and np.array_equal(got["ids"], want["ids"]), (got["ids"].shape, want["ids"].shape)
    bad = np.argwhere(got["cells"] != want["cells"])
    assert len(bad) == 0, (len(bad), bad[:3], got["cells"][tuple(bad[0])], want["cells"][tuple(bad[0])])


def _same_queries(tm, lay, xyz, m, voxel_size):
    dist, cls = tm.distance_query(xyz, m)
    wd, wc = DR.query(lay, xyz, m, voxel_size)
    assert dist.dtype == np.float32 and cls.dtype == np.uint8
    bad = np.flatnonzero((dist.view(np.uint32) != wd.view(np.uint32)) | (cls != wc))
    assert len(bad) == 0, (len(bad), xyz[bad[:3]], m[bad[:3]], dist[bad[:3]], wd[bad[:3]], cls[bad[:3]], wc[bad[:3]])
    return cls


def _blocks_raw(pkg, vo, tm, map_id, capacity):
    import torch
    call = lambda *out: vo._chk(vo.lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, map_id, *out), "vslam_tsdf_distance_blocks_dev")
    ((ids, cells),), (count,) = pkg._read_lists(vo, call, [[(torch.int32, (4,), -9), (torch.uint8, (1024,), 0xAB)]], [capacity])
    return ids, cells.view(np.uint16).reshape(len(ids), 512), count


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_layer_and_queries_equal_the_yardstick(vos, pkg, name, form):
    vo, tm, voxel_size = _map_of(vos, name)
    try:
        before = tm.blocks()
        if DC.cases()[name]["scene"] is not None:
            ids, vox, _ = DC.dump_of(name)
            assert np.array_equal(before[0], ids) and np.array_equal(before[1], vox), "the map the yardstick was fed"
        status = tm.stats()["status"]
        for k, b in enumerate(DC.cases()[name]["builds"]):
            want = DC.reference(name, k)
            got = _build(vo, tm, b, form)
            _same_layer(got, want)
            status |= want["status"]          # (bit 4 stays until the map is cleared, as the other bits do)
            assert tm.stats()["status"] == status, (k, tm.stats()["status"], status)
            xyz, m = DC.query_points(name, k)
            cls = _same_queries(tm, want, xyz, m, voxel_size)
            assert (cls == DR.INVALID).sum() >= 64
            if want["void"]:
                assert ((cls == DR.UNKNOWN) | (cls == DR.INVALID)).all() and tm.last_count == 0
            # (j) a capacity below the count: the full count comes back, `capacity` blocks are written, each one of the layer
            n = want["counts"][1]
            if n >= 2:
                ids, cells, count = _blocks_raw(pkg, vo, tm, b["map_id"], n // 2)
                assert count == n and len(ids) == n // 2
                pos = {tuple(r): i for i, r in enumerate(want["ids"].tolist())}
                rows = [pos[tuple(r)] for r in ids.tolist()]
                assert len(set(rows)) == len(rows) and np.array_equal(cells, want["cells"][rows])
        after = tm.blocks()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the stage writes nothing into the pool"
    finally:
        tm.close()


@pytest.mark.parametrize("name", ["d_random_sparse", "k_narrow", "g_range_edges"])
def test_built_twice_and_in_both_forms_the_bytes_are_equal(vos, name):
    vo, tm, _ = _map_of(vos, name)
    try:
        b = DC.cases()[name]["builds"][-1]
        got = [_build(vo, tm, b, form) for form in (0, 0, 1, 1, 0)]
        for g in got[1:]:
            assert g["counts"] == got[0]["counts"] and g["ids"].tobytes() == got[0]["ids"].tobytes() and g["cells"].tobytes() == got[0]["cells"].tobytes()
    finally:
        tm.close()


def test_tuning_key(vos, pkg):
    vo = vos()
    for v in (0, 1, -1):
        vo.set_tuning(tsdf_dist_form=v)
    with pytest.raises(pkg.VslamError):
        vo.set_tuning(tsdf_dist_form=2)
    vo.set_tuning(tsdf_dist_form=-1)


def _refused(pkg, call):
    with pytest.raises(pkg.VslamError) as e:
        call()
    return str(e.value)


def test_a_changed_map_voids_the_layer_until_it_is_rebuilt(vos, pkg):
    """build; integrate one more frame: both readers are refused; rebuild: both serve the new map's layer.  The same after load_blocks, reintegrate
    and clear."""
    case = TC.cases()["narrow"]
    vo = vos("narrow")
    tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
    R = 5
    pts = np.random.default_rng(4).uniform(-4, 24, (512, 3))

    def fresh():
        got = tm.distance(radius=R, log2_layer_blocks=11)
        want = DR.layer(*tm.blocks(), -1, 1, R, 11)
        _same_layer(got, want)
        _same_queries(tm, want, pts, np.zeros(len(pts), np.int32), case["voxel_size"])
        return got

    def stale():
        assert STALE in _refused(pkg, lambda: _blocks_raw(pkg, vo, tm, -1, 4))
        assert STALE in _refused(pkg, lambda: tm.distance_query(pts))

    try:
        stale()                                   # never built
        _integrate(vo, tm, case, [0, 1])
        stale()
        first = fresh()
        assert first["counts"][0] > 100
        _integrate(vo, tm, case, [2])
        stale()
        second = fresh()
        assert second["counts"] != first["counts"]
        tm.load_blocks(*tm.blocks())
        stale()
        assert fresh()["cells"].tobytes() == second["cells"].tobytes()
        tm.reintegrate(case["disp"][[2]], case["gray"][[2]], case["T"][[2]], None, 0, tm.reach(), case["z_min"], case["z_max"])     # frame 2 taken out
        stale()
        fresh()
        tm.clear()
        stale()
        assert fresh()["counts"] == (0, 0, 0)
    finally:
        tm.close()


def test_bytes_of_the_layer(vos):
    """2257 bytes per block of the layer's table and 64 more, once: counted on the first build, again only for a larger table, returned by destroy"""
    vo = vos()
    start = vo.device_bytes
    c = DC.cases()["b_block_edges"]
    tm = vo.tsdf_map(c["voxel_size"], 4, DC.LOG2_POOL)
    try:
        tm.load_blocks(c["ids"], c["vox"])
        held = vo.device_bytes
        assert held > start
        tm.distance(log2_layer_blocks=10)
        assert vo.device_bytes - held == 2257 * 1024 + 64
        tm.distance(log2_layer_blocks=10)
        tm.distance(log2_layer_blocks=9, radius=3)
        assert vo.device_bytes - held == 2257 * 1024 + 64
        tm.distance(log2_layer_blocks=11)
        assert vo.device_bytes - held == 2257 * 2048 + 64
    finally:
        tm.close()
    assert vo.device_bytes == start


def test_refusals(vos, pkg):
    import torch
    vo = vos()
    lib, err = vo.lib, pkg.VSLAM_ERR_ARG
    c = DC.cases()["a_one_site"]
    tm = vo.tsdf_map(c["voxel_size"], 4, DC.LOG2_POOL)
    other = pkg.VO(device=0, max_batch=2)
    foreign = other.tsdf_map(0.2, 4, 6)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0

    def no(rc, msg):
        assert rc == err and lib.vslam_last_error().decode() == msg, (rc, lib.vslam_last_error().decode(), msg)

    def params(**kw):
        d = dict(struct_size=C.sizeof(pkg.TsdfDistanceParams), map_id=-1, min_weight=1, radius_voxels=8, log2_layer_blocks=10)
        d.update(kw)
        return C.byref(pkg.TsdfDistanceParams(**d))
    try:
        tm.load_blocks(c["ids"], c["vox"])
        who = "vslam_tsdf_distance_dev"
        owner = ": null context or map, or a map of another context"
        no(lib.vslam_tsdf_distance_dev(vo.h, None, params(), None), who + owner)
        no(lib.vslam_tsdf_distance_dev(vo.h, foreign.h, params(), None), who + owner)
        no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, None, None), who + ": null params or struct_size mismatch")
        no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(struct_size=20), None), who + ": null params or struct_size mismatch")
        no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(map_id=-2), None), who + ": map_id -2 outside [-1, 1022]")
        no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(map_id=1023), None), who + ": map_id 1023 outside [-1, 1022]")
        for r in (0, 17, -1):
            no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(radius_voxels=r), None), who + ": radius_voxels %d outside [1, 16]" % r)
        for l2 in (5, 25):
            no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(log2_layer_blocks=l2), None), who + ": log2_layer_blocks %d outside [6, 24]" % l2)
        no(lib.vslam_tsdf_distance_dev(vo.h, tm.h, params(), p + 4), who + ": d_counts must be 8-byte aligned")
        tm.distance()
        who = "vslam_tsdf_distance_blocks_dev"
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, None, -1, p, p + 4096, 1, p + 8192), who + owner)
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, foreign.h, -1, p, p + 4096, 1, p + 8192), who + owner)
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, p, p + 4096, 1, None), who + ": null d_n_out, or a null output with a capacity")
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, None, p + 4096, 1, p + 8192), who + ": null d_n_out, or a null output with a capacity")
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, p, None, 1, p + 8192), who + ": null d_n_out, or a null output with a capacity")
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, 1023, p, p + 4096, 1, p + 8192), who + ": map_id 1023 outside [-1, 1022]")
        align = who + ": d_block_out and d_cells_out must be 16-byte, d_n_out 8-byte aligned"
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, p + 8, p + 4096, 1, p + 8192), align)
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, p, p + 4098, 1, p + 8192), align)
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, p, p + 4096, 1, p + 8196), align)
        assert lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, None, None, 0, p + 8192) == 0, "a counting call"
        who = "vslam_tsdf_distance_query_dev"
        no(lib.vslam_tsdf_distance_query_dev(vo.h, None, p, p + 4096, 4, p + 8192, p + 12288), who + owner)
        no(lib.vslam_tsdf_distance_query_dev(vo.h, foreign.h, p, p + 4096, 4, p + 8192, p + 12288), who + owner)
        for bad in range(4):
            a = [p, p + 4096, p + 8192, p + 12288]
            a[bad] = None
            no(lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, a[0], a[1], 4, a[2], a[3]), who + ": a null pointer with N > 0")
        align = who + ": d_xyz_w must be 8-byte, d_map_id and d_dist 4-byte aligned"
        no(lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, p + 4, p + 4096, 4, p + 8192, p + 12288), align)
        no(lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, p, p + 4098, 4, p + 8192, p + 12288), align)
        no(lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, p, p + 4096, 4, p + 8194, p + 12288), align)
        assert lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, None, None, 0, None, None) == 0, "N == 0 succeeds"
        assert lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, p, p + 4096, 4, p + 8192, p + 12289) == 0, "the class bytes need no alignment"
        vo.sync()
        tm.clear()
        no(lib.vslam_tsdf_distance_blocks_dev(vo.h, tm.h, -1, None, None, 0, p + 8192), "vslam_tsdf_distance_blocks_dev: " + STALE)
        no(lib.vslam_tsdf_distance_query_dev(vo.h, tm.h, None, None, 0, None, None), "vslam_tsdf_distance_query_dev: " + STALE)
        assert np.array_equal(tm.distance()["ids"], np.zeros((0, 4), np.int32)), "an empty map succeeds"
    finally:
        vo.sync()
        tm.close()
        foreign.close()
        other.close()
