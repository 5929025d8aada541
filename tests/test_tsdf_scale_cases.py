"""CPU: the inputs of tests/tsdf_scale_cases.py held to what makes each of them a test -- the many-frame calls decide with the margin of
tests/test_tsdf_ref.py, every word of 64 frames changes the answer, both maps own blocks and the planted poses are the skipped frames; the long lists
pass 4096 entries with real blocks on both sides of it, and the cull's items pass its 4 x 4096 waves likewise; the heavy field stays below 2^32 and crosses; the scene at the limit steps over 2^20; the
regrown map grows.  The device is held to the same references by tests/test_gpu_tsdf_scale.py."""
import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_mesh_ref as MR
import tsdf_scale_cases as SC
from test_tsdf_ref import MARGIN_FLOOR


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("n", SC.FRAME_COUNTS)
def test_many_frames(n):
    case, ref = SC.many_frames(n), SC.many_reference(n)
    assert case["disp"].shape == (n, 48, 37) and SC.MAX_BATCH >= max(SC.FRAME_COUNTS) and (SC.MAX_BATCH + 63) // 64 == 5
    bad = SC.planted(n)
    print(n, "margin %.3g" % ref.margin, "blocks", len(ref.blocks), "decided samples", ref.n_decided, "surfels", len(ref.extract()), len(ref.extract(min_weight=n // 8)))
    assert ref.margin >= MARGIN_FLOOR, ref.margin
    assert ref.n_frames_skipped == len(bad) and ref.status == 4 and ref.n_dropped_range == 0
    assert all(not np.isfinite(case["T"][b]).all() and case["map_id"][b] >= 0 for b in bad)
    if n >= 128:
        assert min(bad) >= 64 and (n < 260 or max(bad) >= 256)
    assert {k[0] for k in ref.blocks} == {0, 3} and (case["map_id"] == -1).any()
    assert SC.min_weights(n) == (1, n // 8, 3 * n // 16, n // 4)
    assert [len(ref.extract(min_weight=m)) > 100 for m in SC.min_weights(n)] == [True, True, True, False], "n // 4 is empty in this scene: 3 n // 16 carries it"
    # every word of 64 frames matters: it holds a frame that takes part and faces the scene (a whole word also one that looks away), and without it
    # the answer is another
    full = ref.dump()
    live = [b for b in range(n) if case["map_id"][b] >= 0 and b not in bad]
    for wd in range((n + 63) // 64):
        assert any(b // 64 == wd and not SC.away(b) for b in live) and (64 * wd + 64 > n or any(b // 64 == wd and SC.away(b) for b in live)), wd
        keep = [b for b in range(n) if b // 64 != wd]
        assert not _same(TC.reference(case, frames=keep).dump(), full), wd
    # the frames that look away claim blocks of their own: those (block, frame) pairs are what the cull drops
    front = TC.reference(case, frames=[b for b in range(n) if not SC.away(b)])
    assert 0 < len(front.blocks) < len(ref.blocks)
    assert 0 < SC.pairs_visited(case, ref)


def test_the_permutation_moves_frames_between_words():
    p = SC.word_permutation(130)
    assert sorted(p.tolist()) == list(range(130)) and (p // 64 != np.arange(130) // 64).sum() > 40
    case = SC.many_frames(130)
    assert _same(TC.reference(case, frames=p).dump(), SC.many_reference(130).dump()), "the rule does not depend on the order of the frames"


def test_cull_second_trip():
    """more (list entry, word) items than the cull kernel has waves, with blocks of the call on both sides of that line"""
    loads, (ids, vox), n_list = SC.cull_second_trip()
    case, ref = SC.many_frames(260), SC.many_reference(260)
    words, waves = (len(case["disp"]) + 63) // 64, SC.CULL_WAVES * SC.GRID
    assert words == 5 and n_list * words > waves and n_list < 1 << SC.LOG2_BLOCKS
    early, pad = loads
    assert len(early[0]) + len(pad[0]) == SC.GRID + 4 and not early[1].any() and not pad[1].any()
    assert len(early[0]) * words < waves < (len(early[0]) + len(pad[0])) * words, "the early blocks' items fall in the first trip, the claimed blocks' in the second"
    late = set(ref.blocks) - {tuple(k) for k in early[0].tolist()}
    assert len(late) >= 20 and {k[0] for k in late} == {0, 3} == set(early[0][:, 0].tolist())
    assert n_list == len(early[0]) + len(pad[0]) + len(late) == len(ids)
    # preset with the loads, the restatement gives the stated answer, and the padding adds no surfel
    pre = SC.with_blocks(np.concatenate([early[0], pad[0]]), np.concatenate([early[1], pad[1]]), case["voxel_size"], case["J"], case["cam"])
    got = TC.reference(case, ref=pre)
    assert _same(got.dump(), (ids, vox)) and SC.pairs_visited(case, got) == SC.pairs_visited(case, ref)
    assert got.extract().tobytes() == ref.extract().tobytes()


def test_long_list():
    first, pad, last = SC.long_list()
    assert len(first[0]) == 26 and len(first[0]) + len(pad[0]) == SC.GRID and len(last[0]) == 27
    ids, vox = SC.long_union()
    assert len(np.unique(ids, axis=0)) == len(ids) == SC.GRID + 27 and len(ids) < 1 << SC.LOG2_BLOCKS
    assert (pad[0][:, 0] == SC.PAD_MAP).all() and pad[0][:, 1:].min() >= 100 and not pad[1].any()
    # the filtered answers are the committed cases' own, but for the map id
    assert _same(SC.long_mesh(0), MC.reference_of("noise_holes"))
    v5, t5 = SC.long_mesh(5)
    want_v, want_t = MC.reference_of("noise_full")
    want_v = want_v.copy(); want_v["map"] = 5
    assert _same((v5, t5), (want_v, want_t))
    # the whole: the two side by side (the padding holds nothing), the triangles of map 5 behind the vertices of map 0
    v, t = SC.long_mesh()
    v0, t0 = SC.long_mesh(0)
    assert v.tobytes() == v0.tobytes() + v5.tobytes() and len(t) == len(t0) + len(t5) and len(t0) > 1000 and len(t5) > 1000
    assert SC.with_blocks(ids, vox, MC.VOXEL_SIZE, 1, (1.0, 1.0, 0.0, 0.0, 1.0)).extract(5).tobytes() == v5.tobytes()


def test_scene_with_padding_passes_the_grid_and_claims_in_the_second_call():
    one, two = SC.scene_padded_reference()
    print("blocks after the first call", len(one.blocks), "after the second", len(two.blocks), "padding", SC.scene_pad())
    assert SC.GRID + 1 == len(one.blocks) and len(one.blocks) < len(two.blocks) < 1 << SC.LOG2_BLOCKS and SC.scene_pad() > 3000
    # the padding changes nothing of the scene: the restatement of the two calls without it
    plain = TC.reference(TC.cases()["scene"], calls=SC.SCENE_SPLIT)
    got = two.dump()
    sel = got[0][:, 0] != SC.PAD_MAP
    assert _same((got[0][sel], got[1][sel]), plain.dump()) and (~sel).sum() == SC.scene_pad()
    assert two.margin >= MARGIN_FLOOR


@pytest.mark.parametrize("over", [False, True])
def test_heavy_field(over):
    c = SC.heavy(over)
    W, Sq = c["voxels"][..., 0].astype(np.int64), c["voxels"][..., 1].astype(np.int64)
    assert W.min() == 1 << 19 and (W == SC.MAX_W).sum() == int(over) and W.max() == (SC.MAX_W if over else SC.MAX_W - 1)
    assert Sq.max() < 2 ** 32 and Sq.max() >= 1024 * (SC.MAX_W - 1) + 1024 * ((SC.MAX_W - 1) // 2), "the largest sum the field's rule gives: 1.5 * 2^30"
    assert Sq.min() == 512 << 19 and (Sq > 2 ** 30).mean() > 0.1
    v, t = SC.heavy_mesh(over)
    s, status = SC.surfels_and_status(c["ids"], c["voxels"], c["voxel_size"])
    print("vertices", len(v), "triangles", len(t))
    assert len(v) > 10000 and len(t) > 20000 and s.tobytes() == v.tobytes()
    assert status & 2 == (2 if over else 0)
    if over:
        assert len(v) < len(SC.heavy_mesh(False)[0]), "the voxel at the limit takes its edges with it"


def test_noise_holes_holds_weights_at_the_limit():
    c = MC.cases()["noise_holes"]
    assert (c["voxels"][..., 0] == SC.MAX_W).any()
    assert SC.surfels_and_status(c["ids"], c["voxels"], c["voxel_size"])[1] & 2


def test_scene_at_the_limit_steps_over_it():
    ids, vox, ref = SC.scene_at_the_limit()
    W0 = vox[..., 0].astype(np.int64)
    assert set(np.unique(W0).tolist()) == {0, SC.LIMIT_W} and vox[..., 1].astype(np.int64).max() < 2 ** 32
    got_ids, got = ref.dump()
    assert np.array_equal(got_ids[np.isin(got_ids.view("i4,i4,i4,i4").ravel(), ids.view("i4,i4,i4,i4").ravel())], ids), "the loaded blocks are all still there"
    W = got[..., 0].astype(np.int64)
    for w in (SC.LIMIT_W, SC.MAX_W - 1, SC.MAX_W):
        assert (W == w).sum() > 100, w
    assert ((W > 0) & (W < SC.LIMIT_W)).sum() > 100, "voxels only the later frames saw"
    s, status = SC.surfels_and_status(got_ids, got, 0.2)
    assert status & 2 and len(s) > 500 and s["weight"].max() == SC.MAX_W - 1
    # a voxel at 2^20 is not good: fewer surfels than the limit lifted by one would give
    below = got.copy()
    below[..., 0][W == SC.MAX_W] = SC.MAX_W - 1
    assert len(s) < len(SC.surfels_and_status(got_ids, below, 0.2)[0])
    assert ref.margin >= MARGIN_FLOOR


def test_regrown_map_grows():
    c = MC.cases()
    ids, vox = SC.regrown()
    assert len(ids) == 35 > len(c["two_maps"]["ids"]) == 16
    v, t = MR.mesh(ids, vox, MC.VOXEL_SIZE)
    assert len(t) > len(MC.reference_of("two_maps")[1]) > 0 and set(v["map"].tolist()) == {0, 5}


@pytest.mark.parametrize("name", ["narrow", "random", "random_step1"])
def test_small_paths(name):
    case = SC.small(name)
    ref, dark = SC.small_reference(name), SC.small_reference(name, with_gray=False)
    assert ref.margin >= MARGIN_FLOOR and dark.margin == ref.margin
    a, b = ref.dump(), dark.dump()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][..., :3], b[1][..., :3]) and a[1][..., 3].any() and not b[1][..., 3].any()
    s = dark.extract()
    assert len(s) > 20 and not s["intensity"].view(np.uint32).any(), "+0.0, not -0.0"
    if name == "random_step1":
        assert case["step"] == 1 and case["disp"].shape[2] == 131 and len(ref.blocks) > len(SC.small_reference("random").blocks)
    if name == "narrow":
        assert case["step"] == 1 and case["disp"].shape[2] == 37
