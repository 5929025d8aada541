"""CPU: the clearance layer's yardstick tests/tsdf_distance_ref.py against hand-worked numbers, against a second, dense statement of the definition,
against scipy's exact Euclidean transform where scipy is installed, and against the geometry of the rendered scene; dense.clearance_slice on a
hand-made layer; and the C-ABI of the stage as far as it can be checked without a device."""
import os
import re

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_distance_cases as DC
import tsdf_distance_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX_LO, BOX = -8, 40          # the dense statements' box: voxel indices [-8, 32)^3 around the random sparse field's 24^3


def _cell(lay, m, v):
    """the cell word of voxel v of map m in a layer() (FAR | UNKNOWN outside it)"""
    table = {tuple(k): c for k, c in zip(lay["ids"].tolist(), lay["cells"])}
    blk = table.get((m, v[0] >> 3, v[1] >> 3, v[2] >> 3))
    return DR.FAR if blk is None else int(blk[(v[2] & 7) << 6 | (v[1] & 7) << 3 | (v[0] & 7)])


def test_one_site_by_hand():
    around = sorted((x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0))
    for b, R, blocks in ((0, 7, around), (1, 8, sorted(around + [(1, 0, 0), (0, 1, 0), (0, 0, 1)]))):
        lay = DC.reference("a_one_site", b)
        assert lay["sites"][0].tolist() == [[0, 0, 0]] and not lay["void"]
        for v, n2 in DC.ONE_SITE_NORM2.items():
            assert _cell(lay, 0, v) & 0xFFF == (n2 if n2 <= R * R else DR.FAR), (R, v)
        assert _cell(lay, 0, (0, 0, 0)) >> 12 == DR.OCCUPIED and _cell(lay, 0, (-1, 0, 0)) >> 12 == DR.FREE and _cell(lay, 0, (1, 0, 0)) >> 12 == DR.UNKNOWN
        # two of the ball's blocks are claimed: the site's and its free neighbour's
        assert sorted(map(tuple, lay["ids"][:, 1:].tolist())) == blocks
        assert lay["counts"] == (1, len(blocks), len(blocks) - 2)
        near = sum(int(((c & 0xFFF) != DR.FAR).sum()) for c in lay["cells"])
        assert near == len(DR.ball(R)[0]) == {7: 1419, 8: 2109}[R], "every voxel of the ball, nothing else"
    dist, cls = DR.query(lay, [(0.1, 0.1, 0.1), (-0.1, 0.1, 0.1), (0.7, -0.9, 0.1), (5.0, 5.0, 5.0), (np.nan, 0, 0), (1e9, 0, 0)], [0, 0, 0, 0, 0, 0], DC.VS)
    vs = np.float64(np.float32(DC.VS))
    assert cls.tolist() == [DR.OCCUPIED, DR.FREE, DR.UNKNOWN, DR.UNKNOWN, DR.INVALID, DR.INVALID]
    assert dist[0] == 0 and not np.signbit(dist[0]) and dist[1] == np.float32(vs) and dist[2] == np.float32(np.sqrt(np.float64(9 + 25)) * vs)
    assert np.isposinf(dist[3:]).all()
    assert DR.query(lay, [(0.1, 0.1, 0.1)], 1, DC.VS)[1][0] == DR.UNKNOWN and DR.query(lay, [(0.1, 0.1, 0.1)], 1023, DC.VS)[1][0] == DR.INVALID


@pytest.mark.parametrize("k", range(4))
def test_separable_trap_by_hand(k):
    """the probe's d2 is the written one: a transform that takes the nearest site per axis instead of the nearest site gets these wrong"""
    for b in (0, 1):
        lay = DC.reference("d_trap_%d" % DC.TRAP_D2[k], b)
        assert lay["counts"][0] == 4 - k
        assert _cell(lay, 0, DC.PROBE) & 0xFFF == DC.TRAP_D2[k]


def test_not_a_site_by_hand():
    for b, min_w in ((0, 1), (1, 2), (2, 1)):     # (a min_weight of 0 counts as 1)
        lay = DC.reference("f_not_a_site", b)
        assert lay["sites"][0].tolist() == [list(s) for s in DC.NOT_A_SITE_EXPECT[min_w]], min_w
        assert _cell(lay, 0, (30, 2, 2)) >> 12 == DR.UNKNOWN, "a weight at 2^20 is not good"
        assert _cell(lay, 0, (2, 2, 2)) >> 12 == (DR.OCCUPIED if min_w == 1 else DR.UNKNOWN)
        assert _cell(lay, 0, (2, 2, 2)) & 0xFFF == DR.FAR, "an occupied voxel with no free neighbour is no site, and none is within 4 voxels"
        assert _cell(lay, 0, (11, 2, 2)) == ((DR.FREE << 12 | 1) if min_w == 1 else (DR.UNKNOWN << 12 | DR.FAR))


def test_edges_void_and_empty():
    lay = DC.reference("g_range_edges", 1)
    assert not lay["void"] and lay["counts"][0] == 3
    assert np.abs(lay["ids"][:, 1:]).max() <= 1 << 14 and lay["ids"][:, 1:].max() == (1 << 14) - 1 and lay["ids"][:, 1:].min() == -(1 << 14)
    pts = DC.cases()["g_range_edges"]["points"]
    dist, cls = DR.query(lay, pts, 0, DC.VS)
    assert cls[0] == DR.OCCUPIED and dist[0] == 0, "voxel index 2^17 - 1 is queryable"
    assert cls[1] == DR.INVALID and cls[2] == DR.INVALID and cls[4] == DR.INVALID, "2^17 and beyond are not"
    assert DC.reference("h_empty", 0)["counts"] == (0, 0, 0) and len(DC.reference("h_empty", 0)["ids"]) == 0
    for b in (0, 1):
        lay = DC.reference("h_no_site", b)
        assert lay["counts"] == (0, 2, 0) and ((lay["cells"] & 0xFFF) == DR.FAR).all(), "claimed blocks without a site: the layer is those blocks, all FAR"
    void = DC.reference("i_overflow", 0)
    assert void["void"] and void["status"] == 16 and void["counts"] == (1, 0, 0) and len(void["ids"]) == 0
    assert DR.query(void, [(0.1, 0.1, 0.1)], 0, DC.VS)[1][0] == DR.UNKNOWN and np.isposinf(DR.query(void, [(0.1, 0.1, 0.1)], 0, DC.VS)[0][0])
    assert not DC.reference("i_overflow", 1)["void"]


def test_two_maps_do_not_see_each_other():
    both, m0, m5 = (DC.reference("e_two_maps", b) for b in range(3))
    for lay, m in ((m0, 0), (m5, 5)):
        sel = both["ids"][:, 0] == m
        assert np.array_equal(both["ids"][sel], lay["ids"]) and np.array_equal(both["cells"][sel], lay["cells"])
    assert np.array_equal(m0["ids"][:, 1:], DC.reference("b_block_edges", 0)["ids"][:, 1:]) and np.array_equal(m0["cells"], DC.reference("b_block_edges", 0)["cells"])
    assert np.array_equal(m0["sites"][0] + [1, 0, 0], m5["sites"][5])


def _dense_box(lay, m):
    """the layer's d2 over the box as a dense (BOX, BOX, BOX) array indexed [x, y, z]"""
    out = np.full((BOX, BOX, BOX), DR.FAR, np.int64)
    for k, c in zip(lay["ids"].tolist(), lay["cells"]):
        if k[0] != m:
            continue
        o = np.array(k[1:]) * 8 - BOX_LO
        if (o < 0).any() or (o + 8 > BOX).any():
            continue
        out[o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8] = (c.reshape(8, 8, 8) & 0xFFF).transpose(2, 1, 0)
    return out


@pytest.mark.parametrize("b", (0, 1))
def test_against_the_dense_statement(b):
    """min over an explicit site list of dx^2 + dy^2 + dz^2, every voxel of a 40^3 box against every site"""
    lay, R = DC.reference("d_random_sparse", b), DC.cases()["d_random_sparse"]["builds"][b]["radius"]
    sites = lay["sites"][0]
    assert 150 <= len(sites) <= 200
    g = np.arange(BOX_LO, BOX_LO + BOX)
    d2 = np.full((BOX, BOX, BOX), 1 << 30, np.int64)
    for s in sites:
        d2 = np.minimum(d2, ((g - s[0]) ** 2)[:, None, None] + ((g - s[1]) ** 2)[None, :, None] + ((g - s[2]) ** 2)[None, None, :])
    want = np.where(d2 <= R * R, d2, DR.FAR)
    assert np.array_equal(_dense_box(lay, 0), want)


def test_both_ways_of_stamping_agree():
    sites = DC.reference("d_random_sparse", 1)["sites"][0]
    for R in (1, 5, 8):
        (ia, da), (ib, db) = DR.stamp(sites, R), DR.stamp(sites, R, dense_limit=0)
        oa, ob = np.lexsort(ia.T[::-1]), np.lexsort(ib.T[::-1])
        assert np.array_equal(ia[oa], ib[ob]) and np.array_equal(da[oa], db[ob])


@pytest.mark.parametrize("b", (0, 1))
def test_against_scipy_edt(b):
    ndi = pytest.importorskip("scipy.ndimage")
    lay, R = DC.reference("d_random_sparse", b), DC.cases()["d_random_sparse"]["builds"][b]["radius"]
    grid = np.ones((BOX, BOX, BOX), bool)
    s = lay["sites"][0] - BOX_LO
    grid[s[:, 0], s[:, 1], s[:, 2]] = False
    d2 = np.rint(ndi.distance_transform_edt(grid) ** 2).astype(np.int64)
    assert np.array_equal(_dense_box(lay, 0), np.where(d2 <= R * R, d2, DR.FAR))


def _plane_distance(scene, p):
    """distance of world points p (n, 3) to the nearest plane of a synth.Scene: the ground, the wall rectangles, the backdrop"""
    d = np.minimum(np.abs(p[:, 1] - scene.ground_y), np.abs(p[:, 2] - scene.back_z))
    for z, x0, x1, y0, y1 in scene.walls:
        dx = np.maximum(np.maximum(x0 - p[:, 0], p[:, 0] - x1), 0)
        dy = np.maximum(np.maximum(y0 - p[:, 1], p[:, 1] - y1), 0)
        d = np.minimum(d, np.sqrt(dx * dx + dy * dy + (p[:, 2] - z) ** 2))
    return d


def test_clearance_against_the_scene_geometry():
    """The four-frame plane scene at R = 8: sqrt(d2) of the FREE voxels within R against the distance of the voxel's centre to the nearest plane of the
    scene, in voxels.  A site is the centre of the voxel on the OCCUPIED end of a crossing edge, so it lies up to one voxel behind the surface and
    anywhere across it: the layer may show a surface up to about one voxel diagonal (sqrt(3) = 1.73) nearer or farther than it is, and farther
    without bound where the nearest part of a plane was never observed.  Measured on this scene (4298 voxels): geometric - clearance at most 1.477;
    clearance - geometric median 0.476, 90th percentile 0.995, maximum 4.750 (unobserved wall edges).  The first bounds are the diagonal; the last line holds the scene to the measured figures, rounded up."""
    scene = TC.scene_frames(4, 7)[0]
    lay = DC.reference("k_scene", 1)
    assert DC.cases()["k_scene"]["builds"][1]["radius"] == 8
    vs = np.float64(np.float32(0.2))
    idx = (lay["ids"][:, None, 1:].astype(np.int64) * 8 + DR._LOCAL[None]).reshape(-1, 3)
    word = lay["cells"].reshape(-1)
    sel = ((word >> 12) == DR.FREE) & ((word & 0xFFF) != DR.FAR)
    c = np.sqrt((word[sel] & 0xFFF).astype(np.float64))               # clearance, voxels
    g = _plane_distance(scene, (idx[sel] + 0.5) * vs) / vs            # the geometry's, voxels
    over = c - g                                                       # > 0: the layer sees the surface farther than it is (an unobserved part of a plane)
    print("free voxels within R %d  geometric - clearance: max %.3f  clearance - geometric: median %.3f  p90 %.3f  max %.3f voxels"
          % (sel.sum(), (-over).max(), np.median(over), np.quantile(over, 0.9), over.max()))
    assert sel.sum() > 4000
    diag = np.sqrt(3.0)
    assert (-over).max() <= diag, "the layer never shows a surface more than a voxel diagonal nearer than the geometry has it"
    assert np.quantile(over, 0.9) <= diag and np.median(np.abs(over)) <= 1.0
    # the measured values, as a guard: this scene, this yardstick (the maximum of clearance - geometric, 4.750, is the unobserved edge of a wall and
    # is left to the 90th percentile)
    assert (-over).max() <= 1.5 and np.quantile(over, 0.9) <= 1.0 and np.median(over) <= 0.5


def test_clearance_slice(pkg):
    from stereo_visual_slam_amd.dense import clearance_slice
    far = np.uint16(DR.FAR)
    ids = np.array([[0, 0, 0, 0], [0, 1, 0, 2], [3, 0, 0, 0]], np.int32)
    cells = np.full((3, 512), far, np.uint16)

    def put(blk, x, y, z, word):
        cells[blk, (z & 7) << 6 | (y & 7) << 3 | (x & 7)] = word
    put(0, 1, 2, 3, 9 | DR.FREE << 12)          # voxel (1, 2, 3)
    put(0, 1, 5, 3, 4 | DR.FREE << 12)          # the same column along y, nearer
    put(0, 1, 7, 3, 1 | DR.OCCUPIED << 12)      # the same column, outside [0, 6)
    put(1, 2, 0, 1, 0 | DR.OCCUPIED << 12)      # voxel (10, 0, 17)
    put(2, 0, 0, 0, 0 | DR.OCCUPIED << 12)      # another map
    s = clearance_slice(ids, cells, 0.2, axis=1, lo=0, hi=6, map_id=0)
    assert s["axes"] == (0, 2) and s["origin"] == (0, 0) and s["d2"].shape == (16, 24) and s["d2"].dtype == np.uint16
    assert s["d2"][1, 3] == 4 and not s["occupied"][1, 3] and s["d2"][10, 17] == 0 and s["occupied"][10, 17]
    assert (s["d2"] != far).sum() == 2 and s["occupied"].sum() == 1
    full = clearance_slice(ids, cells, 0.2, axis=1, lo=0, hi=8, map_id=0)
    assert full["d2"][1, 3] == 1 and full["occupied"][1, 3]
    every = clearance_slice(ids, cells, 0.2, axis=1, lo=0, hi=8)
    assert every["d2"][0, 0] == 0 and every["occupied"][0, 0]
    z = clearance_slice(ids, cells, 0.2, axis=2, lo=16, hi=24, map_id=0)
    assert z["axes"] == (0, 1) and z["origin"] == (8, 0) and z["d2"].shape == (8, 8) and z["d2"][2, 0] == 0 and z["occupied"][2, 0]
    none = clearance_slice(ids, cells, 0.2, axis=1, lo=100, hi=101)
    assert none["d2"].shape == (0, 0)


def test_abi_of_the_stage(pkg):
    """the three entries are declared, exported and in the signature table, their kernels are on the profiler's list and the library knows the tuning
    key (vslam_set_tuning itself needs a context, hence a device: tests/test_gpu_tsdf_distance.py sets the key)"""
    names = ["vslam_tsdf_distance_dev", "vslam_tsdf_distance_blocks_dev", "vslam_tsdf_distance_query_dev"]
    hdr = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = pkg.load_library()
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in pkg.SIGNATURES and n in pkg.ABI_SYMBOLS and hasattr(lib, n), n
    import ctypes as C
    assert C.sizeof(pkg.TsdfDistanceParams) == 24
    kernels = lib.vslam_kernel_names().decode().split()
    assert {"tsdf_dist_classify_kernel", "tsdf_dist_row_kernel", "tsdf_dist_pass_kernel", "tsdf_dist_brute_kernel", "tsdf_dist_query_kernel"} <= set(kernels)
    blob = open(lib._name, "rb").read()
    assert b"tsdf_dist_form\0" in blob and b"VSLAM_TSDF_DIST_FORM\0" in blob
    # argument checks need no device: a null context is refused before anything else
    dp = pkg.TsdfDistanceParams(struct_size=24, map_id=-1, min_weight=1, radius_voxels=8, log2_layer_blocks=10)
    assert lib.vslam_tsdf_distance_dev(None, None, C.byref(dp), None) == pkg.VSLAM_ERR_ARG
    assert lib.vslam_last_error().decode() == "vslam_tsdf_distance_dev: null context or map, or a map of another context"


def test_yardstick_is_quick_enough():
    """the scenes' layers at R = 8 were computed above or are computed here: each within ten seconds on a CPU"""
    import time
    for name in ("k_scene", "k_narrow"):
        ids, vox, _ = DC.dump_of(name)
        t0 = time.perf_counter()
        lay = DR.layer(ids, vox, -1, 1, 8, 12)
        dt = time.perf_counter() - t0
        print("%s: %d claimed blocks, %d sites, %d layer blocks, %.2f s" % (name, len(ids), lay["counts"][0], lay["counts"][1], dt))
        assert not lay["void"] and lay["counts"][0] > 100
        assert dt < 10.0
