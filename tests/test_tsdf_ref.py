"""CPU: the surface map's rule as tests/tsdf_ref.py restates it (include/vslam_hip.h "surface map") -- voxels and a surfel worked by hand, the
margin every committed case decides with, and two properties of the rule itself (it finds the surface; later views carve a phantom), which the
device inherits through the bit equality tests/test_gpu_tsdf.py holds it to."""
import math

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_ref as TR

MARGIN_FLOOR = 1e-9


def test_hand_worked_plane():
    """one camera 5 cm off the origin (no identity pose) in front of a plane at depth 4.1 m; every number below in Python floats, by the header's lines"""
    cam = TC.CAM
    fx, fy, cx, cy, b = cam
    vs = float(np.float32(0.2)); J = 2; tau = J * vs; kq = 1024.0 / tau
    z0 = 4.1
    d = np.float32(fx * b / z0)
    z = fx * b / float(d)                                  # the depth every pixel measures
    T = np.array([[0, 0, 0, 1, 0.013, -0.021, 0.057]], np.float64)
    disp = np.full((1, TC.H, TC.W), d, np.float32)
    gray = np.full((1, TC.H, TC.PITCH), 77, np.uint8)
    ref = TR.TsdfRef(0.2, J, cam)
    ref.integrate(disp, gray, T, np.zeros(1, np.int32), 1.0, 10.0)
    assert ref.n_frames_skipped == 0 and ref.n_dropped_range == 0 and len(ref.blocks) > 4
    # the voxel column (1, -1, iz) of the block the plane's band claims (iz 16 .. 23): in front of the plane, across it, behind it
    want = {}
    for iz in range(16, 24):
        X = [(1 + 0.5) * vs, (-1 + 0.5) * vs, (iz + 0.5) * vs]
        P = [X[0] + 0.013, X[1] - 0.021, X[2] + 0.057]
        u = fx * (P[0] / P[2]) + cx; v = fy * (P[1] / P[2]) + cy
        assert 0 <= math.floor(u + 0.5) < TC.W and 0 <= math.floor(v + 0.5) < TC.H
        sdf = z - P[2]
        if sdf < -tau:
            want[iz] = (0, 0, 0, 0)
            continue
        q = round(min(sdf, tau) * kq)                      # (Python rounds half to even, as rint does)
        want[iz] = (1, q + 1024, 1, 77) if sdf <= tau else (1, q + 1024, 0, 0)
    got = {iz: tuple(int(x) for x in ref.voxel(0, 1, -1, iz)) for iz in want}
    assert got == want, (got, want)
    assert want[16] == (1, 2048, 0, 0) and want[23] == (0, 0, 0, 0), "the column starts in free space beyond tau and ends behind the surface"
    # the one crossing of the column: between the last voxel in front (num > 0) and the first behind
    ia = max(iz for iz, w in want.items() if w[0] and w[1] - 1024 > 0)
    Da, Db = float(want[ia][1] - 1024), float(want[ia + 1][1] - 1024)
    assert Da > 0 > Db
    t = Da / (Da - Db)
    s = ref.extract()
    hit = s[(s["ix"] == 1) & (s["iy"] == -1) & (s["axis"] == 2)]
    assert len(hit) == 1 and hit["iz"][0] == ia and hit["weight"][0] == 1 and hit["intensity"][0] == 77.0
    assert hit["z"][0] == np.float32((ia + 0.5 + t) * vs) and hit["x"][0] == np.float32(1.5 * vs) and hit["y"][0] == np.float32(-0.5 * vs)
    assert abs(float(hit["z"][0]) - (z - 0.057)) < tau / 1024 + 1e-6, "the crossing lies on the plane to within the quantisation step"
    assert (hit["nx"][0], hit["ny"][0], hit["nz"][0]) == (0.0, 0.0, -1.0), "a fronto-parallel plane: the normal looks back along z at the observer"
    assert not len(s[s["axis"] != 2]), "a plane across z crosses no x or y edge"


@pytest.mark.parametrize("name", sorted(TC.cases()))
def test_margin_guard(name):
    """every decision of every committed case is taken at least 1e-9 from its boundary: a device that differs from numpy in the last bits of an f64
    quotient still decides alike.  (A seed that fails is changed, not the floor.)"""
    ref = TC.reference_of(name)
    ids, vox = ref.dump()
    print(name, "margin %.3g" % ref.margin, "blocks", len(ids), "decided samples", ref.n_decided, "surfels", len(ref.extract()))
    assert ref.n_decided > 1000 and len(ids) > 20 and len(ref.extract()) > 20
    assert ref.margin >= MARGIN_FLOOR, ref.margin


def test_cases_cover_what_they_are_for():
    c = TC.cases()
    ids = lambda n: TC.reference_of(n).dump()[0]
    assert (ids("below_zero_j1")[:, 1:] < 0).all(), "every block coordinate below zero"
    assert {c["below_zero_j1"]["J"], c["j8_step3"]["J"]} == {1, 8}
    assert TC.reference_of("random").n_frames_skipped == 0 and np.isnan(c["random"]["disp"]).any() and (c["random"]["disp"] == 0).any()
    assert c["narrow"]["disp"].shape[2] == 37
    assert 150 < len(ids("scene")) < 1500


def _plane_distance(scene, p):
    """distance of world points p (n, 3) to the nearest plane of a synth.Scene: the ground, the wall rectangles, the backdrop"""
    d = np.minimum(np.abs(p[:, 1] - scene.ground_y), np.abs(p[:, 2] - scene.back_z))
    for z, x0, x1, y0, y1 in scene.walls:
        dx = np.maximum(np.maximum(x0 - p[:, 0], p[:, 0] - x1), 0)
        dy = np.maximum(np.maximum(y0 - p[:, 1], p[:, 1] - y1), 0)
        d = np.minimum(d, np.sqrt(dx * dx + dy * dy + (p[:, 2] - z) ** 2))
    return d


def test_accuracy_on_the_scene():
    """the four-frame 160 x 48 scene at 0.2 m voxels, J = 3, gates 2 - 25 m, min_weight 2: the surfels lie on the scene's planes"""
    case = TC.cases()["scene"]
    assert (case["voxel_size"], case["J"], case["z_min"], case["z_max"], len(case["disp"])) == (0.2, 3, 2.0, 25.0, 4)
    scene = TC.scene_frames(4, 7)[0]
    s = TC.reference_of("scene").extract(min_weight=2)
    assert len(s) > 500
    d = _plane_distance(scene, np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float64)) / 0.2
    print("surfels %d  median %.4f voxel  within half a voxel %.1f %%" % (len(s), np.median(d), 100 * (d < 0.5).mean()))
    assert np.median(d) < 0.1
    assert (d < 0.5).mean() >= 0.90


def test_carving():
    """a 10 x 8 px patch of frame 0 set to 6 m: surfels at the patch from that frame alone, none once the other three frames look through it"""
    case = dict(TC.cases()["scene"])
    fx, fy, cx, cy, b = case["cam"]
    r0, c0 = 34, 70
    disp = case["disp"].copy()
    disp[0, r0:r0 + 8, c0:c0 + 10] = np.float32(fx * b / 6.0)
    case["disp"] = disp
    assert (fx * b / TC.cases()["scene"]["disp"][0, r0:r0 + 8, c0:c0 + 10]).min() > 6.0 + 3 * 0.2, "the true surface lies beyond the patch's truncation band"
    R = TR.rotmat(case["T"][0]).reshape(3, 3); t = case["T"][0, 4:]

    def at_patch(s):
        P = np.stack([s["x"], s["y"], s["z"]], 1).astype(np.float64) @ R.T + t
        u = fx * P[:, 0] / P[:, 2] + cx; v = fy * P[:, 1] / P[:, 2] + cy
        return s[(np.abs(P[:, 2] - 6.0) < 0.2) & (u > c0 - 0.5) & (u < c0 + 9.5) & (v > r0 - 0.5) & (v < r0 + 7.5)]

    alone = TC.reference(case, frames=[0])
    assert len(at_patch(alone.extract(min_weight=1))) >= 3, "(at 6 m the patch spans 2.5 x 2 voxels) the phantom is a surface while only its own frame has seen it"
    full = TC.reference(case)
    for min_weight in (1, 2):
        left = at_patch(full.extract(min_weight=min_weight))
        print("min_weight", min_weight, "surfels left at the patch", len(left))
        assert len(left) == 0


def test_surfel_ply_round_trip(tmp_path):
    from stereo_visual_slam_amd.dense import read_ply, read_surfel_ply, write_surfel_ply
    s = TC.reference_of("narrow").extract()
    path = str(tmp_path / "surface.ply")
    write_surfel_ply(path, s)
    back = read_surfel_ply(path)
    assert len(back) == len(s) > 100 and back.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "intensity", "weight")
    for f in back.dtype.names:
        assert np.array_equal(back[f].view(np.uint32), s[f].view(np.uint32)), f
    with pytest.raises(AssertionError):
        read_ply(path)    # (the voxel reader does not take a surfel file for a voxel file)
