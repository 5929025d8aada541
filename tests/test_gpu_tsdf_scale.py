"""GPU: the surface map at the sizes KeyframePipeline.surface_map() runs at, which tests/test_gpu_tsdf.py and tests/test_gpu_tsdf_mesh.py (at most
four frames, max_batch = 8, pools of at most 1024 slots, weights to 10) never reach.  Every comparison is exact, against tests/tsdf_ref.py and
tests/tsdf_mesh_ref.py over the inputs of tests/tsdf_scale_cases.py (held to their purpose on the CPU by tests/test_tsdf_scale_cases.py).  The paths
each size exists for:

1. more than one frame-mask word: calls of 64, 65, 130 and 260 frames on a context with max_batch = 260 (frame_words = 5) -- tsdf_cull_kernel's
   split of (list entry, word), b = 64 word + lane, the b < B guard of a last partial word (65, 130, 260), the stride frame_words above a call's
   words (the 3-frame case on the same context), tsdf_integrate_kernel<true>'s walk over the words, tsdf_frames_kernel's second trip (260 > 256);
2. more than one block per workgroup: lists longer than the 4096 workgroups of the kernels that walk them, in a pool of 2^13 slots -- both
   integrate forms, extract, blocks, mesh vertex and mesh triangle with real blocks on both trips of a workgroup (LDS staged anew behind the
   "readers of the last block are done" barrier), and the loader's second trip (more than 4096 blocks in one call).  The cull kernel walks
   (list entry, word) items with four waves per workgroup: its second trip needs entries x words > 16384, which 4123 entries x 5 words of the
   260-frame call give (test_more_cull_items_than_waves);
3. weights of 2^19 .. 2^20 - 1 in tsdf_num / tsdf_D / the intensity quotient, status bit 2 from the extraction and from the mesh each on its own,
   integration across 2^20;
4. the mesh's vertex-id table reserved anew when the map has grown between two mesh calls;
5. integration without intensities (d_gray = NULL), and the allocation's pixel-by-pixel loads (step 1, disparities 4 bytes past a 16-byte boundary)."""
import functools

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_mesh_ref as MR
import tsdf_scale_cases as SC
from test_gpu_tsdf import _dev, _same_blocks, _same_surfels
from test_gpu_tsdf_mesh import _same_mesh

pytestmark = pytest.mark.gpu
FORMS = [0, 1]


@pytest.fixture(scope="module")
def ctx(pkg):
    """one context per (camera, image size, max_batch): the stage reads the camera from the context"""
    made = {}

    def get(case, max_batch=8):
        key = (case["cam"], case["disp"].shape[1:], max_batch)
        if key not in made:
            made[key] = pkg.VO(device=0, max_batch=max_batch, cam=case["cam"], img_w=case["disp"].shape[2], img_h=case["disp"].shape[1])
        return made[key]

    yield get
    for v in made.values():
        v.close()


@pytest.fixture(scope="module")
def many_vo(ctx):
    return ctx(SC.many_frames(64), SC.MAX_BATCH)


def _integrate(vo, tm, case, frames=None, form=None, with_gray=True, off_by_4=False):
    """one call of the case's frames (all, or `frames` in that order) into tm; off_by_4: the disparities start 4 bytes past a 16-byte boundary"""
    import torch
    fr = list(range(len(case["disp"]))) if frames is None else list(frames)
    disp, gray = case["disp"][fr], case["gray"][fr]
    n, h, w = disp.shape
    pitch = gray.shape[2]
    store = torch.zeros(disp.size + 4, dtype=torch.float32, device="cuda")
    assert store.data_ptr() % 16 == 0
    d_disp = store[1:1 + disp.size] if off_by_4 else store[:disp.size]
    d_disp.copy_(torch.from_numpy(np.ascontiguousarray(disp).ravel()))
    assert d_disp.data_ptr() % 16 == (4 if off_by_4 else 0)
    d_gray, d_T, d_map = _dev(gray), _dev(case["T"][fr]), _dev(case["map_id"][fr])
    torch.cuda.synchronize()
    if form is not None:
        vo.set_tuning(tsdf_form=form)
    try:
        tm.integrate_dev(d_disp.data_ptr(), d_gray.data_ptr() if with_gray else None, h * pitch if with_gray else 0, pitch if with_gray else 0, w, h, n,
                         d_T.data_ptr(), d_map.data_ptr(), case["z_min"], case["z_max"], case["step"])
        vo.sync()
    finally:
        vo.set_tuning(tsdf_form=-1)


def _map_of(vo, case, log2_blocks=10):
    return vo.tsdf_map(case["voxel_size"], case["J"], log2_blocks)


# ------------------------------------------------------------------------------------------------------------------------ 1. many frames
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SC.FRAME_COUNTS)
def test_many_frames_in_one_call(many_vo, n, form):
    case, ref = SC.many_frames(n), SC.many_reference(n)
    tm = _map_of(many_vo, case)
    try:
        _integrate(many_vo, tm, case, form=form)
        _same_blocks(tm.blocks(), ref.dump())
        for min_weight in SC.min_weights(n):
            _same_surfels(tm.extract(min_weight=min_weight), ref.extract(min_weight=min_weight))
        st = tm.stats()
        want = dict(n_blocks=len(ref.blocks), n_samples=ref.n_samples, n_dropped_range=ref.n_dropped_range, n_dropped_full=0, n_frames_skipped=ref.n_frames_skipped,
                    status=4, n_pairs_visited=SC.pairs_visited(case, ref))
        assert {k: st[k] for k in want} == want and ref.n_frames_skipped == len(SC.planted(n)), (st, want)
        assert 0 < st["n_pairs_kept"] < st["n_pairs_visited"], st
    finally:
        tm.close()


@pytest.mark.parametrize("n", SC.FRAME_COUNTS)
def test_both_forms_keep_the_same_pairs(many_vo, n):
    """the cull kernel (a lane per frame of a word) and the walk over all frames evaluate one predicate"""
    case = SC.many_frames(n)
    kept = []
    for form in FORMS:
        tm = _map_of(many_vo, case)
        try:
            _integrate(many_vo, tm, case, form=form)
            st = tm.stats()
            kept.append((st["n_pairs_kept"], st["n_pairs_visited"]))
        finally:
            tm.close()
    assert kept[0] == kept[1] and kept[0][0] > 0, kept


@pytest.mark.parametrize("form", FORMS)
def test_three_frames_where_the_masks_have_five_words(many_vo, form):
    """words = 1 < frame_words = 5: a block's mask lies at 5 slot, not at slot"""
    case, ref = TC.cases()["narrow"], TC.reference_of("narrow")
    tm = _map_of(many_vo, case)
    try:
        _integrate(many_vo, tm, case, form=form)
        _same_blocks(tm.blocks(), ref.dump())
        _same_surfels(tm.extract(), ref.extract())
        st = tm.stats()
        assert (st["status"], st["n_pairs_visited"]) == (0, 3 * len(ref.blocks)), st
    finally:
        tm.close()


@pytest.mark.parametrize("form", FORMS)
def test_frames_moved_between_words_give_the_same_bytes(many_vo, form):
    case = SC.many_frames(130)
    a, b = _map_of(many_vo, case), _map_of(many_vo, case)
    try:
        _integrate(many_vo, a, case, form=form)
        _integrate(many_vo, b, case, frames=SC.word_permutation(130), form=form)
        got = a.blocks()
        _same_blocks(b.blocks(), got)
        _same_blocks(got, SC.many_reference(130).dump())
        _same_surfels(b.extract(), a.extract())
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------------ 2. long lists
@pytest.fixture(scope="module")
def long_map(vo):
    """noise_holes, padding up to list position 4095, noise_full from 4096: three loads, so that the claim order is the list order"""
    tm = vo.tsdf_map(MC.VOXEL_SIZE, 3, SC.LOG2_BLOCKS)
    for ids, vox in SC.long_list():
        tm.load_blocks(ids, vox)
    yield tm
    tm.close()


def _sorted(ids, vox):
    order = np.lexsort((ids[:, 3], ids[:, 2], ids[:, 1], ids[:, 0]))
    return ids[order], vox[order]


def test_long_list_blocks_are_the_loaded_bytes(long_map):
    ids, vox = SC.long_union()
    st = long_map.stats()
    assert (st["n_blocks"], st["n_dropped_range"], st["n_dropped_full"], st["status"]) == (SC.GRID + 27, 0, 0, 0), st
    _same_blocks(long_map.blocks(), _sorted(ids, vox))
    for m, n in ((0, 26), (5, 27), (SC.PAD_MAP, SC.GRID - 26)):
        got = long_map.blocks(map_id=m)
        assert len(got[0]) == n
        _same_blocks(got, _sorted(ids[ids[:, 0] == m], vox[ids[:, 0] == m]))


@pytest.mark.parametrize("map_id", [-1, 0, 5])
def test_long_list_mesh_and_surfels(long_map, map_id):
    """workgroup g < 26 meshes block g of noise_holes, then block g of noise_full (list position 4096 + g) with the same LDS"""
    want = SC.long_mesh(map_id)
    got = long_map.mesh(map_id=map_id)
    assert long_map.last_counts == (len(want[0]), len(want[1])) and len(want[1]) > 1000
    _same_mesh(got, want)
    _same_surfels(long_map.extract(map_id=map_id), want[0])
    assert long_map.stats()["status"] & 1 == 0


def test_more_blocks_in_one_load_than_workgroups(vo, long_map):
    ids, vox = SC.long_union()
    assert len(ids) > SC.GRID
    tm = vo.tsdf_map(MC.VOXEL_SIZE, 3, SC.LOG2_BLOCKS)
    try:
        tm.load_blocks(ids, vox)
        st = tm.stats()
        assert (st["n_blocks"], st["n_dropped_range"], st["n_dropped_full"], st["status"]) == (len(ids), 0, 0, 0), st
        _same_blocks(tm.blocks(), long_map.blocks())
        one, three = tm.mesh(), long_map.mesh()
        assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes() and len(one[1]) > 1000
    finally:
        tm.close()


def test_more_cull_items_than_waves(many_vo):
    """tsdf_cull_kernel takes 4 x 4096 (list entry, word) items a trip: 4123 entries x 5 words of 260 frames need a second one, and the blocks the
    call claims lie there (the masks the second trip writes decide their voxels); half the call's blocks are claimed beforehand, in the first"""
    case, ref = SC.many_frames(260), SC.many_reference(260)
    loads, want, n_list = SC.cull_second_trip()
    assert n_list * 5 > SC.CULL_WAVES * SC.GRID
    kept = []
    for form in (1, 0):
        tm = _map_of(many_vo, case, SC.LOG2_BLOCKS)
        try:
            for ids, vox in loads:
                tm.load_blocks(ids, vox)
            assert tm.stats()["n_blocks"] == SC.GRID + 4
            _integrate(many_vo, tm, case, form=form)
            _same_blocks(tm.blocks(), want)
            for min_weight in SC.min_weights(260)[:3]:
                _same_surfels(tm.extract(min_weight=min_weight), ref.extract(min_weight=min_weight))
            st = tm.stats()
            expect = dict(n_blocks=n_list, n_samples=ref.n_samples, n_dropped_range=0, n_dropped_full=0, n_frames_skipped=2, status=4,
                          n_pairs_visited=SC.pairs_visited(case, ref))
            assert {k: st[k] for k in expect} == expect, (st, expect)
            assert 0 < st["n_pairs_kept"] < st["n_pairs_visited"], st
            kept.append(st["n_pairs_kept"])
        finally:
            tm.close()
    assert kept[0] == kept[1], kept


@functools.lru_cache(maxsize=None)
def _scene_padded_yardsticks():
    ref = SC.scene_padded_reference()[1]
    ids, vox = ref.dump()
    return (ids, vox), ref.extract(min_weight=2), MR.mesh(ids, vox, TC.cases()["scene"]["voxel_size"])


@pytest.mark.parametrize("form", FORMS)
def test_frames_into_a_loaded_map_past_4096_blocks(ctx, form):
    """two frames, padding up to list position 4096, two more frames: the blocks the second call claims lie beyond the grid, and workgroup g reaches
    them after the first call's block g -- also the loader's save-and-continue use"""
    case = TC.cases()["scene"]
    vo = ctx(case)
    one, two = SC.scene_padded_reference()
    blocks, surfels, mesh = _scene_padded_yardsticks()
    tm = _map_of(vo, case, SC.LOG2_BLOCKS)
    try:
        _integrate(vo, tm, case, frames=SC.SCENE_SPLIT[0], form=form)
        n1 = tm.stats()["n_blocks"]
        assert n1 == len(one.blocks) - SC.scene_pad()
        tm.load_blocks(*SC.padding(SC.scene_pad()))
        assert tm.stats()["n_blocks"] == SC.GRID + 1
        _integrate(vo, tm, case, frames=SC.SCENE_SPLIT[1], form=form)
        st = tm.stats()
        assert st["n_blocks"] == len(two.blocks) > SC.GRID + 1 and (st["n_dropped_full"], st["status"]) == (0, 0), st
        _same_blocks(tm.blocks(), blocks)
        _same_surfels(tm.extract(min_weight=2), surfels)
        _same_mesh(tm.mesh(), mesh)
    finally:
        tm.close()


# ------------------------------------------------------------------------------------------------------------------------ 3. weights at the limit
def _loaded(vo, c, log2_blocks=8):
    tm = vo.tsdf_map(c["voxel_size"], 3, log2_blocks)
    tm.load_blocks(c["ids"], c["voxels"])
    return tm


def test_heavy_field(vo):
    c = SC.heavy()
    want = SC.heavy_mesh()
    tm = _loaded(vo, c)
    try:
        _same_mesh(tm.mesh(), want)
        assert tm.stats()["status"] & 2 == 0
        _same_surfels(tm.extract(), want[0])
        assert tm.stats()["status"] == 0
    finally:
        tm.close()


@pytest.mark.parametrize("field", ["heavy", "noise_holes"])
def test_a_weight_at_the_limit_sets_status_bit_2_in_extract_and_in_mesh(vo, field):
    c = SC.heavy(True) if field == "heavy" else MC.cases()["noise_holes"]
    want = SC.heavy_mesh(True) if field == "heavy" else MC.reference_of("noise_holes")
    assert SC.surfels_and_status(c["ids"], c["voxels"], c["voxel_size"])[1] & 2
    a, b = _loaded(vo, c), _loaded(vo, c)
    try:
        a.clear()
        assert a.stats()["status"] == 0
        a.load_blocks(c["ids"], c["voxels"])
        assert a.stats()["status"] == 0 and b.stats()["status"] == 0, "loading sets nothing"
        _same_surfels(a.extract(), want[0])
        assert a.stats()["status"] & 2, "the extraction"
        _same_mesh(b.mesh(), want)
        assert b.stats()["status"] & 2, "the mesh"
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("form", FORMS)
def test_integration_across_the_weight_limit(ctx, form):
    case = TC.cases()["scene"]
    vo = ctx(case)
    ids, vox, ref = SC.scene_at_the_limit()
    want = ref.dump()
    surfels, status = SC.surfels_and_status(want[0], want[1], case["voxel_size"])
    tm = _map_of(vo, case)
    try:
        tm.load_blocks(ids, vox)
        _integrate(vo, tm, case, frames=[2, 3], form=form)
        got = tm.blocks()
        _same_blocks(got, want)
        assert (got[1][..., 0] >= SC.MAX_W).any() and tm.stats()["status"] == 0
        _same_surfels(tm.extract(), surfels)
        assert status & 2 and tm.stats()["status"] & 2
        _same_mesh(tm.mesh(), MR.mesh(want[0], want[1], case["voxel_size"]))
    finally:
        tm.close()


# ------------------------------------------------------------------------------------------------------------------------ 4. the vertex-id table grows
def test_the_mesh_after_the_map_has_grown(vo):
    c = MC.cases()
    ids, vox = SC.regrown()
    tm = vo.tsdf_map(MC.VOXEL_SIZE, 3, 8)
    table = lambda n_blocks: (1536 * n_blocks + (1 << 8)) * 4
    try:
        before = vo.device_bytes
        tm.load_blocks(c["two_maps"]["ids"], c["two_maps"]["voxels"])
        first = tm.mesh()
        _same_mesh(first, MC.reference_of("two_maps"))
        assert tm.stats()["n_blocks"] == 16 and vo.device_bytes - before == table(16)
        tm.load_blocks(c["noise_full"]["ids"], c["noise_full"]["voxels"])
        assert tm.stats()["n_blocks"] == len(ids) == 35
        _same_mesh(tm.mesh(), MR.mesh(ids, vox, MC.VOXEL_SIZE))
        assert vo.device_bytes - before == table(35)
        for m in (0, 5):
            _same_mesh(tm.mesh(map_id=m), MR.mesh(ids, vox, MC.VOXEL_SIZE, 1, m))
        tm.clear()
        tm.load_blocks(c["two_maps"]["ids"], c["two_maps"]["voxels"])
        again = tm.mesh()
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
        assert vo.device_bytes - before == table(35), "the table does not shrink"
    finally:
        tm.close()


# ------------------------------------------------------------------------------------------------------------------------ 5. small paths
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["random", "narrow"])
def test_without_intensities(ctx, name, form):
    case, ref = SC.small(name), SC.small_reference(name, with_gray=False)
    vo = ctx(case)
    tm = _map_of(vo, case)
    try:
        _integrate(vo, tm, case, form=form, with_gray=False)
        got = tm.blocks()
        _same_blocks(got, ref.dump())
        assert not got[1][..., 3].any() and got[1][..., 2].any()
        s = tm.extract()
        _same_surfels(s, ref.extract())
        assert len(s) > 20 and not s["intensity"].view(np.uint32).any(), "+0.0"
    finally:
        tm.close()


@pytest.mark.parametrize("off_by_4", [False, True])
@pytest.mark.parametrize("name", ["narrow", "random_step1"])
def test_allocation_from_disparities_off_the_16_byte_boundary(ctx, name, off_by_4):
    """step 1: 16-byte row loads from an aligned base, pixel by pixel from one 4 bytes past it (_integrate asserts the residue)"""
    case, ref = SC.small(name), SC.small_reference(name)
    assert case["step"] == 1
    vo = ctx(case)
    tm = _map_of(vo, case)
    try:
        _integrate(vo, tm, case, off_by_4=off_by_4)
        _same_blocks(tm.blocks(), ref.dump())
        st = tm.stats()
        assert (st["n_samples"], st["n_dropped_range"], st["n_dropped_full"], st["status"]) == (ref.n_samples, ref.n_dropped_range, 0, 0), st
        _same_surfels(tm.extract(), ref.extract())
    finally:
        tm.close()
