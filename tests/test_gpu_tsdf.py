"""GPU: the surface map stage (include/vslam_hip.h "surface map") against the numpy restatement tests/tsdf_ref.py, which culls nothing: the raw
blocks (the block set and all four sums of every voxel) and the surfels bit for bit (floats compared as bits), over every case of
tests/tsdf_cases.py in both integration forms; frames permuted, split over calls, held apart by map id, skipped; a pool that overflows; every
refused argument.  Shapes are small (160 x 48 and smaller, at most four frames)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_ref as TR

pytestmark = pytest.mark.gpu
FORMS = [0, 1]


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


@pytest.fixture(scope="module")
def vos(pkg):
    """one context per camera of the cases (the stage reads the camera from the context)"""
    made = {}

    def get(case):
        key = (case["cam"], case["disp"].shape[2])
        if key not in made:
            made[key] = pkg.VO(device=0, max_batch=8, cam=case["cam"], img_w=case["disp"].shape[2], img_h=case["disp"].shape[1])
        return made[key]

    yield get
    for v in made.values():
        v.close()


def _integrate(vo, tm, case, frames=None, form=None):
    """one call of the case's frames (all, or `frames` in that order) into tm"""
    fr = list(range(len(case["disp"]))) if frames is None else list(frames)
    disp, gray = case["disp"][fr], case["gray"][fr]
    n, h, w = disp.shape
    pitch = gray.shape[2]
    d = [_dev(disp), _dev(gray), _dev(case["T"][fr]), _dev(case["map_id"][fr])]
    if form is not None:
        vo.set_tuning(tsdf_form=form)
    try:
        tm.integrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, n, d[2].data_ptr(), d[3].data_ptr(), case["z_min"], case["z_max"], case["step"])
        vo.sync()
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


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(TC.cases()))
def test_blocks_and_surfels_equal_the_restatement(vos, pkg, name, form):
    assert pkg.SURFEL_MAP_DTYPE == TR.SURFEL_MAP_DTYPE and pkg.SURFEL_DTYPE.itemsize == 48
    case = TC.cases()[name]
    ref = TC.reference_of(name)
    vo = vos(case)
    tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
    try:
        _integrate(vo, tm, case, form=form)
        _same_blocks(tm.blocks(), ref.dump())
        st = tm.stats()
        want = dict(n_blocks=len(ref.blocks), n_samples=ref.n_samples, n_dropped_range=ref.n_dropped_range, n_dropped_full=0, n_frames_skipped=0, status=0)
        assert {k: st[k] for k in want} == want, (st, want)
        assert 0 < st["n_pairs_kept"] <= st["n_pairs_visited"] == len(ref.blocks) * len(case["disp"])
        for min_weight in (1, 2):
            _same_surfels(tm.extract(min_weight=min_weight), ref.extract(min_weight=min_weight))
        # a capacity below the count: the full count comes back, `capacity` surfels are written, each one of the list
        full = ref.extract()
        part = tm.extract(capacity=16)
        assert tm.last_count == len(full) and len(part) == 16
        key = lambda s: list(zip(s["map"].tolist(), s["ix"].tolist(), s["iy"].tolist(), s["iz"].tolist(), s["axis"].tolist()))
        pos = {k: i for i, k in enumerate(key(full))}
        _same_surfels(part, full[[pos[k] for k in key(part)]])
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_permuted_frames_give_the_same_bytes(vos, form):
    case = TC.cases()["scene"]
    vo = vos(case)
    a, b = vo.tsdf_map(0.2, case["J"], 10), vo.tsdf_map(0.2, case["J"], 10)
    try:
        _integrate(vo, a, case, form=form)
        _integrate(vo, b, case, frames=[2, 0, 3, 1], form=form)
        _same_blocks(a.blocks(), b.blocks())
        _same_surfels(a.extract(), b.extract())
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("form", FORMS)
def test_two_calls_equal_the_restatement_of_two_calls(vos, form):
    """a call's frames reach the blocks claimed so far, not the ones a later call claims: two calls differ from one, and the restatement says how"""
    case = TC.cases()["scene"]
    two = TC.reference(case, calls=[[0, 1], [2, 3]])
    one = TC.reference_of("scene")
    assert sorted(two.blocks) == sorted(one.blocks) and (two.dump()[1] != one.dump()[1]).any(), "the split must matter in the restatement"
    vo = vos(case)
    tm = vo.tsdf_map(0.2, case["J"], 10)
    try:
        _integrate(vo, tm, case, frames=[0, 1], form=form)
        _integrate(vo, tm, case, frames=[2, 3], form=form)
        _same_blocks(tm.blocks(), two.dump())
        _same_surfels(tm.extract(min_weight=2), two.extract(min_weight=2))
    finally:
        tm.close()


def test_map_ids_are_held_apart_and_a_map_alone_is_the_same(vos):
    base = TC.cases()["scene"]
    case = dict(base, map_id=np.array([0, 1022, 0, 1022], np.int32))
    ref = TC.reference(case)
    assert {k[0] for k in ref.blocks} == {0, 1022}
    vo = vos(case)
    both, alone = vo.tsdf_map(0.2, case["J"], 10), vo.tsdf_map(0.2, case["J"], 10)
    try:
        _integrate(vo, both, case)
        _same_blocks(both.blocks(), ref.dump())
        _same_surfels(both.extract(), ref.extract())
        _integrate(vo, alone, case, frames=[0, 2])
        for m in (0, 1022):
            _same_blocks(both.blocks(map_id=m), ref.dump(map_id=m))
            _same_surfels(both.extract(map_id=m), ref.extract(map_id=m))
        _same_blocks(alone.blocks(), both.blocks(map_id=0))
        _same_surfels(alone.extract(), both.extract(map_id=0))
        assert len(both.extract(map_id=7)) == 0 and len(both.blocks(map_id=7)[0]) == 0
    finally:
        both.close(); alone.close()


@pytest.mark.parametrize("form", FORMS)
def test_frames_without_a_map_or_a_finite_pose_are_skipped(vos, form):
    base = TC.cases()["scene"]
    T = base["T"].copy()
    T[2, 5] = np.nan
    case = dict(base, T=T, map_id=np.array([0, -1, 0, 0], np.int32))
    ref = TC.reference(case)
    assert ref.n_frames_skipped == 1 and ref.status == 4
    _same_blocks(ref.dump(), TC.reference(base, frames=[0, 3]).dump())
    vo = vos(case)
    tm = vo.tsdf_map(0.2, case["J"], 10)
    try:
        _integrate(vo, tm, case, form=form)
        _same_blocks(tm.blocks(), ref.dump())
        st = tm.stats()
        assert st["n_frames_skipped"] == 1 and st["status"] == 4 and st["n_samples"] == ref.n_samples, st
    finally:
        tm.close()


def test_the_same_call_into_a_cleared_map_gives_the_same_dump(vos):
    case = TC.cases()["random"]
    vo = vos(case)
    tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
    zero = dict(n_blocks=0, n_samples=0, n_dropped_range=0, n_dropped_full=0, n_frames_skipped=0, n_pairs_visited=0, n_pairs_kept=0, status=0)
    try:
        assert tm.stats() == zero and len(tm.extract()) == 0 and len(tm.blocks()[0]) == 0
        _integrate(vo, tm, case)
        first, s1, st1 = tm.blocks(), tm.extract(), tm.stats()
        tm.clear()
        assert tm.stats() == zero and len(tm.extract()) == 0 and len(tm.blocks()[0]) == 0
        _integrate(vo, tm, case)
        _same_blocks(tm.blocks(), first)
        _same_surfels(tm.extract(), s1)
        assert tm.stats() == st1
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_a_full_pool_drops_blocks_and_keeps_the_rest_exact(vos, form):
    """64 slots for the scene's blocks: which blocks are lost depends on the arrival order, but integration is a pure function of voxel and frames,
    so every claimed block still equals the restatement's"""
    case = TC.cases()["scene"]
    ref = TC.reference_of("scene")
    assert len(ref.blocks) > 128
    vo = vos(case)
    tm = vo.tsdf_map(0.2, case["J"], 6)
    try:
        _integrate(vo, tm, case, form=form)
        st = tm.stats()
        ids, vox = tm.blocks()
        assert st["n_dropped_full"] > 0 and st["status"] & 1 and st["n_blocks"] == len(ids) <= 64, st
        assert st["n_samples"] + st["n_dropped_full"] == ref.n_samples and len(ids) >= 32
        for k, v in zip(ids.tolist(), vox):
            assert np.array_equal(v, ref.blocks[tuple(k)].astype(np.uint32)), k
        tm.extract()    # (neighbour lookups in a full table end at the probe limit)
    finally:
        tm.close()


def test_the_pool_counts_in_device_bytes(vos, pkg):
    vo = vos(TC.cases()["scene"])
    before = vo.device_bytes
    tm = vo.tsdf_map(0.2, 4, 8)
    assert vo.device_bytes - before >= 8192 << 8
    tm.close()
    assert vo.device_bytes == before
    # a context closes what was created on it: one object of each kind, each counted to the byte, closed by the context, closed again to no effect
    ctx = pkg.VO(device=0, max_batch=1)
    try:
        base = ctx.device_bytes
        vm, tm, db = ctx.voxel_map(0.2, 10), ctx.tsdf_map(0.2, 4, 6), ctx.place_db(rows=32, capacity=4, with_geometry=False)
        table = (32 << 10) + 8 * 8                                            # slots | counters
        pool = ((8192 + 8 + 8 + 4) << 6) + 16 * 8 + 8 * 8                     # per block: voxels, key, one mask word, list entry | one frame | counters
        entries = 4 * 32 * 32 + 3 * 256                                       # descriptors | n, seq, frame, each padded to 256 bytes
        assert ctx.device_bytes == base + table + pool + entries
    finally:
        ctx.close()
    assert vm.h is None and tm.h is None and db.h is None and ctx.h is None
    for obj in (vm, tm, db, ctx):
        obj.close()
    assert vm.h is None and tm.h is None and db.h is None


def test_refused_arguments(vos, pkg):
    import torch
    vo = vos(TC.cases()["scene"])
    lib, ERR = vo.lib, pkg.VSLAM_ERR_ARG
    no = _refusals(lib, ERR, "tsdf")
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    h = C.c_void_p()
    for size, J, log2 in ((0.0, 4, 8), (-0.2, 4, 8), (float("nan"), 4, 8), (float("inf"), 4, 8), (1e-60, 4, 8), (0.2, 0, 8), (0.2, 9, 8), (0.2, -1, 8), (0.2, 4, 5), (0.2, 4, 23)):
        no("create %r %d %d" % (size, J, log2), lib.vslam_tsdf_create(vo.h, size, J, log2, C.byref(h)))
        assert not h.value, (size, J, log2)
    no("create null ctx", lib.vslam_tsdf_create(None, 0.2, 4, 8, C.byref(h)))
    no("create null out", lib.vslam_tsdf_create(vo.h, 0.2, 4, 8, None))
    tm = vo.tsdf_map(0.2, 4, 6)
    other = pkg.VO(device=0, max_batch=1)
    zero = tm.stats()
    try:
        good = dict(d=p, w=16, h=8, B=2, T=p, z0=1.0, z1=50.0, step=1)
        bad = [dict(B=0), dict(B=9), dict(step=0), dict(step=-1), dict(z0=50.0, z1=50.0), dict(z0=60.0), dict(z1=float("nan")), dict(d=None), dict(T=None), dict(w=0), dict(h=0)]
        for kw in bad:
            a = dict(good, **kw)
            no("integrate %r" % kw, lib.vslam_tsdf_integrate_dev(vo.h, tm.h, a["d"], None, 0, 0, a["w"], a["h"], a["B"], a["T"], p, a["z0"], a["z1"], a["step"]))
        run = lambda ctx, m, ids, gray=None, img_bytes=0, pitch=0: lib.vslam_tsdf_integrate_dev(ctx, m, p, gray, img_bytes, pitch, 16, 8, 2, p, ids, 1.0, 50.0, 1)
        no("integrate null d_map_id", run(vo.h, tm.h, None))
        no("integrate null map", run(vo.h, None, p))
        no("integrate null ctx", run(None, tm.h, p))
        no("integrate a map of another context", run(other.h, tm.h, p))
        no("integrate pitch below w", run(vo.h, tm.h, p, gray=p, img_bytes=16 * 8, pitch=15))
        no("integrate img_bytes below pitch * h", run(vo.h, tm.h, p, gray=p, img_bytes=16 * 7, pitch=16))
        for map_id in (-2, 1023):
            no("extract map_id %d" % map_id, lib.vslam_tsdf_extract_dev(vo.h, tm.h, map_id, 1, p, None, 4, p))
            no("blocks map_id %d" % map_id, lib.vslam_tsdf_blocks_dev(vo.h, tm.h, map_id, p, p, 4, p))
        no("extract null d_n_out", lib.vslam_tsdf_extract_dev(vo.h, tm.h, -1, 1, p, None, 4, None))
        no("extract null d_out", lib.vslam_tsdf_extract_dev(vo.h, tm.h, -1, 1, None, None, 4, p))
        no("extract null map", lib.vslam_tsdf_extract_dev(vo.h, None, -1, 1, p, None, 4, p))
        no("extract a map of another context", lib.vslam_tsdf_extract_dev(other.h, tm.h, -1, 1, p, None, 4, p))
        no("blocks null d_n_out", lib.vslam_tsdf_blocks_dev(vo.h, tm.h, -1, p, p, 4, None))
        no("blocks null d_block_out", lib.vslam_tsdf_blocks_dev(vo.h, tm.h, -1, None, p, 4, p))
        no("blocks null d_voxels_out", lib.vslam_tsdf_blocks_dev(vo.h, tm.h, -1, p, None, 4, p))
        no("blocks null map", lib.vslam_tsdf_blocks_dev(vo.h, None, -1, p, p, 4, p))
        no("clear null map", lib.vslam_tsdf_clear(None))
        no("stats null host", lib.vslam_tsdf_stats(tm.h, None))
        no("stats null map", lib.vslam_tsdf_stats(None, C.byref(pkg.TsdfStats())))
        st = pkg.TsdfStats(); st.struct_size = 8
        no("stats struct_size", lib.vslam_tsdf_stats(tm.h, C.byref(st)))
        no("set_tuning tsdf_form 2", lib.vslam_set_tuning(vo.h, b"tsdf_form", 2))
        vo.sync()
        assert tm.stats() == zero and zero["n_blocks"] == 0, "a refused call launches nothing"
    finally:
        tm.close(); other.close()
