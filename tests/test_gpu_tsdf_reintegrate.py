"""GPU: RE-INTEGRATION of the surface map (include/vslam_hip.h "RE-INTEGRATION") against the numpy yardstick tests/tsdf_reintegrate_ref.py, which
culls nothing: every scenario of tests/tsdf_reintegrate_cases.py in both forms of "tsdf_form" -- the raw blocks, the surfels and the status bit for
bit, the reach after every call; mesh and ray-cast views of a moved map against the mesh and render yardsticks on the yardstick's blocks; the moved
frames in one call against two; the host-array entry; the tables' bytes; every refused argument.  Shapes are those of tests/tsdf_cases.py (160 x 48
and smaller, at most four frames) and 65 / 129 frames of 37 x 48."""

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reintegrate_cases as RC

pytestmark = pytest.mark.gpu
FORMS = [0, 1]


def _dev(a):
    import torch
    t = torch.from_numpy(np.array(a)).to("cuda")     # (a copy: the cases' arrays are read-only)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def vos(pkg):
    """one context per camera and batch size of the scenarios (the stage reads the camera from the context)"""
    made = {}

    def get(case):
        n, h, w = case["disp"].shape
        key = (case["cam"], w, 8 if n <= 8 else n)
        if key not in made:
            made[key] = pkg.VO(device=0, max_batch=key[2], cam=case["cam"], img_w=w, img_h=h)
        return made[key]

    yield get
    for v in made.values():
        v.close()


def _u32(reach):
    return np.clip(reach, 0, 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _play(vo, tm, scn, after, form=None, calls=None, start=0):
    """the scenario's calls [start, calls) on the device, the reach checked after each: the yardstick's block count `after`"""
    c = scn["case"]
    _, h, w = c["disp"].shape
    pitch = c["gray"].shape[2]
    if form is not None:
        vo.set_tuning(tsdf_form=form)
    try:
        for k in range(start, len(scn["calls"]) if calls is None else calls):
            call = scn["calls"][k]
            fr = call["frames"]
            d = [_dev(c["disp"][fr]), _dev(c["gray"][fr]), _dev(call["map_id"])]
            if call["kind"] == "integrate":
                T = _dev(call["T"])
                tm.integrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, len(fr), T.data_ptr(), d[2].data_ptr(), c["z_min"], c["z_max"], c["step"])
            else:
                To, Tn, r = _dev(call["T_old"]), _dev(call["T_new"]), _dev(_u32(RC.resolve(call["reach"], after)))
                tm.reintegrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, len(fr), To.data_ptr(), Tn.data_ptr(), d[2].data_ptr(), r.data_ptr(),
                                   c["z_min"], c["z_max"], c["step"])
            assert tm.reach() == after[k] == tm.stats()["n_blocks"], (k, tm.reach(), after[k])
    finally:
        vo.set_tuning(tsdf_form=-1)


def _same_blocks(got, want):
    (gi, gv), (wi, wv) = got, want
    assert gi.shape == wi.shape and np.array_equal(gi, wi), (gi.shape, wi.shape)
    bad = np.argwhere(gv != wv)
    assert len(bad) == 0, (len(bad), bad[:3], gv[tuple(bad[0])], wv[tuple(bad[0])])


def _same_surfels(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (got.dtype, want.dtype, len(got), len(want))
    for f in got.dtype.names:
        bad = np.flatnonzero(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert len(bad) == 0, (f, len(bad), got[bad[:3]], want[bad[:3]])


def _map(vo, scn, log2_blocks=10):
    return vo.tsdf_map(scn["case"]["voxel_size"], scn["case"]["J"], log2_blocks)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(RC.scenarios()))
def test_blocks_surfels_and_status_equal_the_yardstick(vos, name, form):
    scn = RC.scenarios()[name]
    ref, after, under = RC.reference_of(name)
    vo = vos(scn["case"])
    tm = _map(vo, scn)
    try:
        _play(vo, tm, scn, after, form=form)
        _same_blocks(tm.blocks(), ref.dump())
        st = tm.stats()
        want = dict(n_blocks=len(ref.blocks), n_samples=ref.n_samples, n_dropped_range=ref.n_dropped_range, n_dropped_full=0, n_frames_skipped=ref.n_frames_skipped,
                    status=ref.status)
        assert {k: st[k] for k in want} == want, (st, want)
        assert (st["status"] & 8 != 0) == (sum(under) > 0)
        assert 0 < st["n_pairs_kept"] <= st["n_pairs_visited"]
        for min_weight in (1, 2):
            _same_surfels(tm.extract(min_weight=min_weight), ref.extract(min_weight=min_weight))
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_pairs_count_both_sides_alike_in_both_forms(vos, form):
    """move_all of the scene: one map, four frames, nothing culled away from the count of visited pairs -- the integrate call looks at (blocks) x 4
    pairs, the re-integration at min(reach, n0) x 4 old sides and (blocks after its allocation) x 4 new sides"""
    scn = RC.scenarios()["move_all/scene"]
    _, after, _ = RC.reference_of("move_all/scene")
    vo = vos(scn["case"])
    tm = _map(vo, scn)
    try:
        _play(vo, tm, scn, after, form=form)
        st = tm.stats()
        assert st["n_pairs_visited"] == 4 * after[0] + 4 * after[0] + 4 * after[1], (st, after)
        assert 0 < st["n_pairs_kept"] < st["n_pairs_visited"]
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_mesh_and_views_of_a_moved_map(vos, form):
    """the moved scene: mesh() against tests/tsdf_mesh_ref.py and render() from the new poses against tests/tsdf_render_ref.py, both on the yardstick's blocks"""
    import tsdf_mesh_ref as MR
    import tsdf_render_ref as VR
    scn = RC.scenarios()["move_all/scene"]
    c = scn["case"]
    ref, after, _ = RC.reference_of("move_all/scene")
    ids, vox = ref.dump()
    vo = vos(c)
    tm = _map(vo, scn)
    try:
        _play(vo, tm, scn, after, form=form)
        (gv, gt), (wv, wt) = tm.mesh(), MR.mesh(ids, vox, c["voxel_size"])
        assert len(wv) > 1000 and len(wt) > 1000
        _same_surfels(gv, wv)
        assert gt.shape == wt.shape and np.array_equal(gt, wt)
        T = scn["calls"][1]["T_new"][:2]
        size = (c["disp"].shape[2] // 2, c["disp"].shape[1] // 2)
        cam = tuple(v / 2 for v in c["cam"][:4])
        want = VR.render(ids, vox, c["voxel_size"], T, [0, 0], cam, size, c["z_min"], c["z_max"], 0.5)
        got = tm.render(T, 0, K4=cam, size=size, z_min=c["z_min"], z_max=c["z_max"], march=0.5)
        assert want["hits"] > 1000 and got["counts"][0] == want["hits"]
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        assert np.array_equal(bits(got["depth"]), bits(want["depth"]))
        assert np.array_equal(bits(np.concatenate([got["normal"], got["intensity"][..., None]], -1)), bits(want["attr"]))
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_one_call_and_two_calls_agree_on_the_blocks_that_existed(vos, form):
    """the moved frames as one call and split over two with the reach updated between them: every block claimed before the move holds the same bytes
    (a block the second of two calls claims has not seen the first call's frames -- INTEGRATION's own rule for later calls -- and the yardstick says
    how: test_blocks_surfels_and_status_equal_the_yardstick[split_calls])"""
    one, two = RC.scenarios()["move_all/scene"], RC.scenarios()["split_calls"]
    a1, a2 = RC.reference_of("move_all/scene")[1], RC.reference_of("split_calls")[1]
    vo = vos(one["case"])
    A, B = _map(vo, one), _map(vo, two)
    try:
        _play(vo, A, one, a1, form=form)
        _play(vo, B, two, a2, form=form)
        (ia, va), (ib, vb) = A.blocks(), B.blocks()
        assert np.array_equal(ia, ib)
        old = set(TC.reference_of("scene").blocks)
        sel = np.array([tuple(k) in old for k in ia.tolist()])
        assert sel.sum() == a1[0] < len(ia) and np.array_equal(va[sel], vb[sel])
    finally:
        A.close(); B.close()


def test_host_arrays_entry_and_reach(vos):
    """TsdfMap.reintegrate() on numpy arrays and on torch tensors, one map id and one reach for every frame"""
    import torch
    scn = RC.scenarios()["move_all/scene"]
    c, call = scn["case"], scn["calls"][1]
    ref, after, _ = RC.reference_of("move_all/scene")
    vo = vos(c)
    tm = _map(vo, scn)
    try:
        _play(vo, tm, scn, after, calls=1)
        assert tm.reach() == after[0]
        d = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tm.reach_dev(d.data_ptr() + 4)
        vo.sync()
        assert d.cpu().tolist() == [0, after[0]]
        assert tm.reintegrate(c["disp"], c["gray"], call["T_old"], call["T_new"], 0, after[0], c["z_min"], c["z_max"], c["step"]) == after[1]
        _same_blocks(tm.blocks(), ref.dump())
        # back again through tensors, without images: the map's I sums keep the move's intensities, the other three sums return
        back = tm.reintegrate(torch.from_numpy(c["disp"]).cuda(), None, torch.from_numpy(call["T_new"]), call["T_old"], torch.zeros(4, dtype=torch.int32),
                              np.full(4, after[1]), c["z_min"], c["z_max"], c["step"])
        assert back == after[1] and tm.stats()["status"] == 0
        got = dict(zip(map(tuple, tm.blocks()[0].tolist()), tm.blocks()[1]))
        orig = TC.reference_of("scene")
        assert all(np.array_equal(got[k][:, :3], v[:, :3].astype(np.uint32)) for k, v in orig.blocks.items())
    finally:
        tm.close()


def test_the_old_sides_tables_count_in_device_bytes(vos):
    scn = RC.scenarios()["remove_all"]
    _, after, _ = RC.reference_of("remove_all")
    vo = vos(scn["case"])
    empty = vo.device_bytes
    tm = _map(vo, scn, log2_blocks=8)
    try:
        _play(vo, tm, scn, after, calls=1)
        before = vo.device_bytes
        _play(vo, tm, scn, after, start=1)
        grown = vo.device_bytes - before
        assert grown == 8 * 128 + (8 << 8) + 8, grown          # max_batch 8: 128 bytes per frame, one mask word per slot, n0
    finally:
        tm.close()
    assert vo.device_bytes == empty


def test_a_call_of_no_frames_and_refused_arguments(vos, pkg):
    import torch
    vo = vos(TC.cases()["scene"])
    lib, ERR = vo.lib, pkg.VSLAM_ERR_ARG
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    tm = vo.tsdf_map(0.2, 4, 6)
    other = pkg.VO(device=0, max_batch=1)
    zero = tm.stats()
    try:
        def run(**kw):
            a = dict(ctx=vo.h, m=tm.h, d=p, gray=None, img_bytes=0, pitch=0, w=16, h=8, B=2, To=p, Tn=p, ids=p, reach=p, z0=1.0, z1=50.0, step=1)
            a.update(kw)
            return lib.vslam_tsdf_reintegrate_dev(a["ctx"], a["m"], a["d"], a["gray"], a["img_bytes"], a["pitch"], a["w"], a["h"], a["B"], a["To"], a["Tn"], a["ids"], a["reach"],
                                                  a["z0"], a["z1"], a["step"])

        assert run(B=0) == 0 and run(B=0, To=None, Tn=None, reach=None, ids=None, d=None) == 0, "B == 0 is a no-op that succeeds"
        for kw in (dict(To=None), dict(Tn=None), dict(reach=None), dict(ids=None), dict(d=None), dict(B=-1), dict(B=9), dict(step=0), dict(step=-1), dict(z0=50.0, z1=50.0),
                   dict(z0=60.0), dict(z1=float("nan")), dict(w=0), dict(h=0), dict(m=None), dict(ctx=None), dict(ctx=other.h), dict(B=0, m=None), dict(B=0, ctx=other.h),
                   dict(gray=p, img_bytes=16 * 8, pitch=15), dict(gray=p, img_bytes=16 * 7, pitch=16)):
            assert run(**kw) == ERR, kw
        assert lib.vslam_tsdf_reach_dev(vo.h, tm.h, None) == ERR and lib.vslam_tsdf_reach_dev(vo.h, None, p) == ERR and lib.vslam_tsdf_reach_dev(None, tm.h, p) == ERR
        assert lib.vslam_tsdf_reach_dev(other.h, tm.h, p) == ERR and lib.vslam_tsdf_reach_dev(vo.h, tm.h, p + 2) == ERR
        vo.sync()
        assert tm.stats() == zero and zero["n_blocks"] == 0 and vo.device_bytes > 0, "a refused call launches nothing"
        assert tm.reach() == 0
    finally:
        tm.close(); other.close()
