"""GPU: the surface map's mesh (vslam_tsdf_mesh_dev) and block loader (vslam_tsdf_load_blocks_dev) against the numpy yardstick tests/tsdf_mesh_ref.py
over the fields of tests/tsdf_mesh_cases.py: vertices compared as bits, triangles equal, in the canonical form; the vertices against extract() byte
for byte; the map filter; permuted loads and repeated calls; capacities below the counts with canary rows; a scene integrated on the device; the
loader's round trip, full pool and refused ids; every refused argument.  The largest field is 27 blocks of random voxels."""
import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_mesh_ref as MR

pytestmark = pytest.mark.gpu
NAMES = ["noise_full", "noise_holes", "two_maps", "sphere", "scene"]


def _same_mesh(got, want):
    (gv, gt), (wv, wt) = got, want
    assert gv.dtype == wv.dtype and len(gv) == len(wv), (gv.dtype, wv.dtype, len(gv), len(wv))
    for f in gv.dtype.names:
        bad = np.flatnonzero(gv[f].view(np.uint32) != wv[f].view(np.uint32))
        assert len(bad) == 0, (f, len(bad), gv[bad[:3]], wv[bad[:3]])
    assert gt.dtype == np.int32 and gt.shape == wt.shape, (gt.dtype, gt.shape, wt.shape)
    bad = np.flatnonzero((gt != wt).any(1))
    assert len(bad) == 0, (len(bad), gt[bad[:3]], wt[bad[:3]])


def _loaded(vo, name, log2_blocks=8, order=None):
    c = MC.cases()[name]
    tm = vo.tsdf_map(c["voxel_size"], 3, log2_blocks)
    order = np.arange(len(c["ids"])) if order is None else order
    tm.load_blocks(c["ids"][order], c["voxels"][order])
    return tm


@pytest.fixture(scope="module")
def maps(vo):
    """every case loaded once into a map of its own"""
    made = {name: _loaded(vo, name) for name in NAMES}
    yield made
    for tm in made.values():
        tm.close()


@pytest.mark.parametrize("name", NAMES)
def test_load_blocks_then_blocks_returns_the_loaded_bytes(maps, name):
    c = MC.cases()[name]
    ids, vox = maps[name].blocks()
    order = np.lexsort((c["ids"][:, 3], c["ids"][:, 2], c["ids"][:, 1], c["ids"][:, 0]))
    assert np.array_equal(ids, c["ids"][order]) and vox.tobytes() == c["voxels"][order].tobytes()
    st = maps[name].stats()
    assert (st["n_blocks"], st["n_dropped_range"], st["n_dropped_full"], st["status"] & 1) == (len(ids), 0, 0, 0), st


def test_loading_again_replaces_the_voxels_and_claims_nothing(vo):
    c = MC.cases()["two_maps"]
    tm = _loaded(vo, "two_maps")
    try:
        other = np.ascontiguousarray(c["voxels"][::-1])
        tm.load_blocks(c["ids"][:3], other[:3])
        ids, vox = tm.blocks()
        assert tm.stats()["n_blocks"] == len(c["ids"]) == len(ids)
        want = c["voxels"].copy()
        want[:3] = other[:3]
        order = np.lexsort((c["ids"][:, 3], c["ids"][:, 2], c["ids"][:, 1], c["ids"][:, 0]))
        assert vox.tobytes() == want[order].tobytes()
    finally:
        tm.close()


def test_a_full_pool_drops_and_counts_and_keeps_the_rest_exact(vo):
    """100 blocks into 64 slots: 64 are held, every one with its own bytes, 36 are counted"""
    rng = np.random.default_rng(3)
    ids = np.concatenate([np.zeros((100, 1), np.int32), rng.permutation(1000)[:100, None].astype(np.int32) - 500, rng.integers(-50, 50, (100, 2)).astype(np.int32)], 1)
    vox = rng.integers(0, 1 << 32, (100, 512, 4), dtype=np.uint64).astype(np.uint32)
    tm = vo.tsdf_map(0.2, 3, 6)
    try:
        tm.load_blocks(ids, vox)
        st = tm.stats()
        got_ids, got_vox = tm.blocks()
        assert st["n_blocks"] == len(got_ids) == 64 and st["n_dropped_full"] == 36 and st["status"] & 1, st
        where = {tuple(k): i for i, k in enumerate(ids.tolist())}
        for k, v in zip(got_ids.tolist(), got_vox):
            assert np.array_equal(v, vox[where[tuple(k)]]), k
        tm.mesh()   # (neighbour lookups in a full table end at the probe limit)
    finally:
        tm.close()


def test_ids_out_of_range_are_refused_per_block(vo):
    c = MC.cases()["two_maps"]
    bad = np.array([[-1, 0, 0, 0], [1023, 0, 0, 0], [0, 1 << 14, 0, 0], [0, 0, -(1 << 14) - 1, 0], [0, 0, 0, 1 << 20], [1 << 20, 0, 0, 0]], np.int32)
    edge = np.array([[1022, (1 << 14) - 1, -(1 << 14), 0], [0, -(1 << 14), (1 << 14) - 1, (1 << 14) - 1]], np.int32)
    ids = np.concatenate([bad[:3], edge, bad[3:]])
    tm = vo.tsdf_map(0.2, 3, 6)
    try:
        tm.load_blocks(ids, c["voxels"][:len(ids)])
        st = tm.stats()
        assert (st["n_blocks"], st["n_dropped_range"], st["n_dropped_full"], st["status"]) == (2, len(bad), 0, 0), st
        got_ids, got_vox = tm.blocks()
        assert sorted(got_ids.tolist()) == sorted(edge.tolist())
        for k, v in zip(got_ids.tolist(), got_vox):
            assert np.array_equal(v, c["voxels"][ids.tolist().index(k)])
        # blocks at the last coordinate have no neighbour beyond it: the mesh of each equals the yardstick's of the block alone
        _same_mesh(tm.mesh(), MR.mesh(got_ids, got_vox, 0.2))
    finally:
        tm.close()


@pytest.mark.parametrize("min_weight", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_mesh_equals_the_yardstick_and_its_vertices_equal_extract(maps, name, min_weight):
    tm = maps[name]
    want = MC.reference_of(name, min_weight)
    got = tm.mesh(min_weight=min_weight)
    assert tm.last_counts == (len(want[0]), len(want[1])), (tm.last_counts, len(want[0]), len(want[1]))
    _same_mesh(got, want)
    assert got[0].tobytes() == tm.extract(min_weight=min_weight).tobytes()
    if len(want[1]):
        assert got[1].min() >= 0 and got[1].max() < len(got[0])


def test_the_map_filter(maps):
    tm = maps["two_maps"]
    for m in (0, 5):
        _same_mesh(tm.mesh(map_id=m), MC.reference_of("two_maps", 1, m))
    v, t = tm.mesh(map_id=7)
    assert len(v) == 0 and len(t) == 0 and tm.last_counts == (0, 0)


def test_unsorted_output_is_a_mesh_of_its_own(maps, pkg):
    """sort=False returns the device's order: indices into the device's vertex array, the same mesh once brought to the canonical form"""
    tm = maps["noise_holes"]
    v, t = tm.mesh(sort=False)
    assert t.min() >= 0 and t.max() < len(v)
    _same_mesh(pkg.canonical_mesh(v, t), MC.reference_of("noise_holes"))


@pytest.mark.parametrize("name", ["noise_holes", "two_maps"])
def test_permuted_loads_and_repeated_calls_give_the_same_canonical_bytes(vo, maps, name):
    first = maps[name].mesh()
    again = maps[name].mesh()
    order = np.random.default_rng(5).permutation(len(MC.cases()[name]["ids"]))
    tm = _loaded(vo, name, log2_blocks=7, order=order)
    try:
        other = tm.mesh()
    finally:
        tm.close()
    for m in (again, other):
        assert m[0].tobytes() == first[0].tobytes() and m[1].tobytes() == first[1].tobytes()


def test_capacities_below_the_counts(vo, maps, pkg):
    """the full counts come back, nothing at or beyond a capacity is touched (canary rows), every written row is one of the full answer's"""
    import torch
    tm = maps["noise_holes"]
    full_v, full_t = MC.reference_of("noise_holes")
    vcap, tcap, extra = 1000, 700, 64
    d_v = torch.full((vcap + extra, 48), 0xA5, dtype=torch.uint8, device="cuda")
    d_m = torch.full((vcap + extra,), -77, dtype=torch.int32, device="cuda")
    d_t = torch.full((tcap + extra, 3), -77, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    # (a) both below: the triangle indices are not meaningful, the vertex rows are
    vo._chk(vo.lib.vslam_tsdf_mesh_dev(vo.h, tm.h, -1, 1, d_v.data_ptr(), d_m.data_ptr(), vcap, d_t.data_ptr(), tcap, d_n.data_ptr()), "vslam_tsdf_mesh_dev")
    vo.sync()
    assert d_n.cpu().tolist() == [len(full_v), len(full_t)] and len(full_v) > vcap and len(full_t) > tcap
    assert (d_v[vcap:].cpu().numpy() == 0xA5).all() and (d_m[vcap:].cpu().numpy() == -77).all() and (d_t[tcap:].cpu().numpy() == -77).all()
    rows = d_v[:vcap].cpu().numpy().reshape(-1).view(pkg.SURFEL_DTYPE)
    key = lambda s: list(zip(s["ix"].tolist(), s["iy"].tolist(), s["iz"].tolist(), s["axis"].tolist()))
    pos = {k: i for i, k in enumerate(key(full_v))}
    idx = [pos[k] for k in key(rows)]
    assert len(set(idx)) == vcap
    for f in pkg.SURFEL_DTYPE.names:
        assert np.array_equal(rows[f].view(np.uint32), full_v[f][idx].view(np.uint32)), f
    assert (d_m[:vcap].cpu().numpy() == 0).all()
    assert (d_t[:tcap].cpu().numpy() != -77).all(), "every row below the capacity is written"
    # (b) the vertices fit, the triangles do not: every written triangle is one of the full answer's
    d_v2 = torch.zeros((len(full_v), 48), dtype=torch.uint8, device="cuda")
    d_m2 = torch.zeros(len(full_v), dtype=torch.int32, device="cuda")
    d_t.fill_(-77)
    torch.cuda.synchronize()
    vo._chk(vo.lib.vslam_tsdf_mesh_dev(vo.h, tm.h, -1, 1, d_v2.data_ptr(), d_m2.data_ptr(), len(full_v), d_t.data_ptr(), tcap, d_n.data_ptr()), "vslam_tsdf_mesh_dev")
    vo.sync()
    assert d_n.cpu().tolist() == [len(full_v), len(full_t)] and (d_t[tcap:].cpu().numpy() == -77).all()
    rows = d_v2.cpu().numpy().reshape(-1).view(pkg.SURFEL_DTYPE)
    to_full = np.array([pos[k] for k in key(rows)], np.int32)
    part = to_full[d_t[:tcap].cpu().numpy()]
    have = {tuple(r) for r in full_t.tolist()}
    assert len({tuple(r) for r in part.tolist()}) == tcap and all(tuple(r) in have for r in part.tolist())
    # (c) a counting call writes nothing but the counts
    vo._chk(vo.lib.vslam_tsdf_mesh_dev(vo.h, tm.h, -1, 1, None, None, 0, None, 0, d_n.data_ptr()), "vslam_tsdf_mesh_dev")
    vo.sync()
    assert d_n.cpu().tolist() == [len(full_v), len(full_t)]


def test_a_scene_integrated_on_the_device_then_meshed(pkg):
    """the blocks are the integration's own, in the order it claimed them, not loaded"""
    import torch
    case = TC.cases()["scene"]
    vo = pkg.VO(device=0, max_batch=8, cam=case["cam"], img_w=case["disp"].shape[2], img_h=case["disp"].shape[1])
    try:
        empty = vo.device_bytes
        tm = vo.tsdf_map(case["voxel_size"], case["J"], 10)
        n, h, w = case["disp"].shape
        pitch = case["gray"].shape[2]
        d = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (case["disp"], case["gray"], case["T"], case["map_id"])]
        torch.cuda.synchronize()
        before = vo.device_bytes
        tm.integrate_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, n, d[2].data_ptr(), d[3].data_ptr(), case["z_min"], case["z_max"], case["step"])
        vo.sync()
        for min_weight in (1, 2):
            _same_mesh(tm.mesh(min_weight=min_weight), MC.reference_of("scene", min_weight))
        # the vertex-id table is the map's, sized by the claimed blocks and counted while the map lives
        n_blocks = tm.stats()["n_blocks"]
        assert vo.device_bytes - before == (1536 * n_blocks + (1 << 10)) * 4
        tm.mesh()
        assert vo.device_bytes - before == (1536 * n_blocks + (1 << 10)) * 4, "a second call grows nothing"
        tm.close()
        assert vo.device_bytes == empty
    finally:
        vo.close()


def test_refused_arguments(vo, pkg):
    import torch
    lib, ERR = vo.lib, pkg.VSLAM_ERR_ARG
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    tm = vo.tsdf_map(0.2, 4, 6)
    other = pkg.VO(device=0, max_batch=1)
    zero = tm.stats()
    try:
        mesh = lambda ctx=vo.h, m=tm.h, map_id=-1, v=p, vm=p, vcap=4, t=p, tcap=4, n=p: lib.vslam_tsdf_mesh_dev(ctx, m, map_id, 1, v, vm, vcap, t, tcap, n)
        assert mesh(n=None) == ERR and mesh(v=None) == ERR and mesh(t=None) == ERR
        assert mesh(m=None) == ERR and mesh(ctx=None) == ERR and mesh(ctx=other.h) == ERR, "a map of another context"
        assert mesh(map_id=-2) == ERR and mesh(map_id=1023) == ERR
        assert mesh(v=p + 4) == ERR and mesh(vm=p + 2) == ERR and mesh(t=p + 2) == ERR and mesh(n=p + 4) == ERR, "alignment"
        load = lambda ctx=vo.h, m=tm.h, ids=p, vox=p, n=1: lib.vslam_tsdf_load_blocks_dev(ctx, m, ids, vox, n)
        assert load(ids=None) == ERR and load(vox=None) == ERR and load(m=None) == ERR and load(ctx=None) == ERR and load(ctx=other.h) == ERR
        assert load(ids=p + 4) == ERR and load(vox=p + 8) == ERR, "alignment"
        vo.sync()
        assert tm.stats() == zero and zero["n_blocks"] == 0, "a refused call launches nothing"
        assert load(ids=None, vox=None, n=0) == 0 and tm.stats() == zero, "an empty list is no error"
        # a negative min_weight counts as 1, as in the extraction
        assert lib.vslam_tsdf_mesh_dev(vo.h, tm.h, -1, -5, None, None, 0, None, 0, p) == 0
        vo.sync()
    finally:
        tm.close(); other.close()
