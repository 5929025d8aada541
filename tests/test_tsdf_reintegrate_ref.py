"""CPU: RE-INTEGRATION as tests/tsdf_reintegrate_ref.py restates it (include/vslam_hip.h "RE-INTEGRATION") -- a voxel column worked by hand, the
margin every scenario of tests/tsdf_reintegrate_cases.py decides with, and the properties that make the bit equality of
tests/test_gpu_tsdf_reintegrate.py mean something: moving every frame gives a fresh map's sums, removing them gives zeros, reach is what keeps a
frame out of blocks it never reached, and a frame taken out twice is refused voxel by voxel."""
import math

import numpy as np
import pytest

import tsdf_cases as TC
import tsdf_reintegrate_cases as RC
import tsdf_reintegrate_ref as RR

MARGIN_FLOOR = 1e-9     # the stage's floor (tests/test_tsdf_ref.py)


def _blocks_equal_on(ref, other):
    """the voxels in which ref differs from other, over other's blocks (all of which ref must hold)"""
    return sum(int((ref.blocks[k] != v).any(-1).sum()) for k, v in other.blocks.items())


def test_hand_worked_column():
    """the plane of tests/test_tsdf_ref.py's hand-worked case, seen from t = (0.013, -0.021, 0.057) and moved to t' = (0.013, -0.021, 0.257): the column
    (1, -1, iz) after the move holds what the header's lines give at t' alone, and nothing after the removal; every number in Python floats"""
    cam = TC.CAM
    fx, fy, cx, cy, b = cam
    vs = float(np.float32(0.2)); J = 2; tau = J * vs; kq = 1024.0 / tau
    d = np.float32(fx * b / 4.1)
    z = fx * b / float(d)
    t_old, t_new = (0.013, -0.021, 0.057), (0.013, -0.021, 0.257)
    T_old = np.array([[0, 0, 0, 1, *t_old]], np.float64); T_new = np.array([[0, 0, 0, 1, *t_new]], np.float64)
    disp = np.full((1, TC.H, TC.W), d, np.float32)
    gray = np.full((1, TC.H, TC.PITCH), 77, np.uint8)
    ids = np.zeros(1, np.int32)

    def column(t):
        want = {}
        for iz in range(14, 24):
            X = [(1 + 0.5) * vs, (-1 + 0.5) * vs, (iz + 0.5) * vs]
            P = [X[0] + t[0], X[1] + t[1], X[2] + t[2]]
            u = fx * (P[0] / P[2]) + cx; v = fy * (P[1] / P[2]) + cy
            assert P[2] > vs and 0 <= math.floor(u + 0.5) < TC.W and 0 <= math.floor(v + 0.5) < TC.H
            sdf = z - P[2]
            if sdf < -tau:
                want[iz] = (0, 0, 0, 0)
                continue
            q = round(min(sdf, tau) * kq)
            want[iz] = (1, q + 1024, 1, 77) if sdf <= tau else (1, q + 1024, 0, 0)
        return want

    ref = RR.TsdfReintRef(0.2, J, cam)
    ref.integrate(disp, gray, T_old, ids, 1.0, 10.0)
    reach = ref.reach()
    assert reach == len(ref.blocks) > 4
    held = lambda iz: (0, 0, -1, iz >> 3) in ref.blocks       # (a voxel in no block reads as zeros: compare where a block holds it)
    old, new = column(t_old), column(t_new)
    assert old != new and {iz: tuple(int(x) for x in ref.voxel(0, 1, -1, iz)) for iz in old if held(iz)} == {iz: w for iz, w in old.items() if held(iz)}
    assert ref.reintegrate(disp, gray, T_old, T_new, ids, [reach], 1.0, 10.0) == 0 and ref.status == 0
    assert ref.reach() >= reach
    got = {iz: tuple(int(x) for x in ref.voxel(0, 1, -1, iz)) for iz in new if held(iz)}
    assert sum(held(iz) for iz in new) >= 8 and got == {iz: w for iz, w in new.items() if held(iz)}, (got, new)
    n = ref.reach()
    assert ref.reintegrate(disp, gray, T_new, np.full((1, 7), np.nan), ids, [n], 1.0, 10.0) == 0
    assert ref.reach() == n and all(not v.any() for v in ref.blocks.values()) and len(ref.extract()) == 0


@pytest.mark.parametrize("name", sorted(RC.scenarios()))
def test_margin_guard(name):
    """every decision of every scenario -- at the old poses and at the new ones -- is taken at least 1e-9 from its boundary.  (A seed that fails is
    changed, not the floor.)"""
    ref, after, under = RC.reference_of(name)
    print(name, "margin %.3g" % ref.margin, "blocks after each call", after, "underflowed", under)
    assert ref.margin >= MARGIN_FLOOR, ref.margin
    assert (sum(under) > 0) == (name == "remove_twice") and (ref.status & RR.UNDERFLOW != 0) == (name == "remove_twice")


@pytest.mark.parametrize("name", sorted(TC.cases()))
def test_move_all_equals_a_fresh_map_at_the_new_poses(name):
    scn = RC.scenarios()["move_all/" + name]
    ref, after, _ = RC.reference_of("move_all/" + name)
    new = RC.fresh(scn, scn["calls"][1]["T_new"])
    assert after[1] >= after[0] > 20 and set(new.blocks) <= set(ref.blocks)
    assert _blocks_equal_on(ref, new) == 0
    a, b = ref.extract(), new.extract()
    assert len(a) == len(b) > 20 and a.tobytes() == b.tobytes()
    old = RC.fresh(scn, scn["case"]["T"])
    assert any((ref.blocks[k] != v).any() for k, v in old.blocks.items()), "the move must matter"


def test_remove_all_leaves_claimed_zeros():
    ref, after, _ = RC.reference_of("remove_all")
    assert after[1] == after[0] == len(ref.blocks) > 100
    assert all(not v.any() for v in ref.blocks.values()) and len(ref.extract()) == 0


def test_reach_keeps_a_frame_out_of_blocks_it_never_reached():
    scn = RC.scenarios()["two_calls_remove_first"]
    ref, after, _ = RC.reference_of("two_calls_remove_first")
    assert after[0] < after[1] == after[2]
    alone = RC.fresh(scn, scn["case"]["T"], frames=[1, 2, 3])
    assert set(alone.blocks) <= set(ref.blocks) and _blocks_equal_on(ref, alone) == 0
    # the guard that the scenario can catch a kernel that ignores reach: with the final block count in reach's place the map differs, and silently
    blind, _, under = RC.run(scn, ignore_reach=True)
    differ = sum(int((blind.blocks[k] != v).any(-1).sum()) for k, v in ref.blocks.items())
    print("voxels that differ with the reach ignored:", differ)
    assert differ >= 50 and under[-1] == 0 and blind.status == 0


def test_mixed_call_is_the_sum_of_its_parts():
    """the mixed call against fresh maps: on map 0's first blocks, frame 0 at its new pose alone (frame 1 is gone); map 1 keeps frames 2 and 3 at their
    old and new pose and gains frame 0's image at a pose of its own"""
    scn = RC.scenarios()["mixed"]
    c, call = scn["case"], scn["calls"][1]
    ref, after, _ = RC.reference_of("mixed")
    assert {k[0] for k in ref.blocks} == {0, 1} and after[1] > after[0]
    want0 = RC.fresh(scn, np.stack([call["T_new"][0]] * 4), frames=[0], map_id=np.zeros(1, np.int32))
    assert _blocks_equal_on(ref, want0) == 0
    T1 = np.stack([call["T_new"][4], c["T"][1], call["T_new"][2], call["T_new"][5]])
    want1 = RC.fresh(scn, T1, frames=[0, 2, 3], map_id=np.ones(3, np.int32))
    first, _, _ = RC.run(scn, calls=1)
    same = [k for k in want1.blocks if k in first.blocks]         # (blocks of the first call received every frame of map 1)
    assert len(same) > 20 and all((ref.blocks[k] == want1.blocks[k]).all() for k in same)


def test_reach_edges_cut_where_they_should():
    scn = RC.scenarios()["reach_edges"]
    ref, after, under = RC.reference_of("reach_edges")
    before, _, _ = RC.run(scn, calls=2)
    keys = list(before.blocks)
    assert after[0] < after[1] == after[2] == len(keys) and under[2] == 0
    # frame 1 (reach 0) is still in, frame 3 (reach above the list) is out everywhere, frame 2 is out of the first call's blocks only
    first, later = keys[:after[0]], keys[after[0]:]
    f01, f12, f1 = (RC.sums_on(scn, keys, fr) for fr in ([0, 1], [1, 2], [1]))
    assert all((ref.blocks[k] == f01[k]).all() for k in first), "the first call's blocks: frames 0 and 1 remain"
    assert all((ref.blocks[k] == f12[k]).all() for k in later), "the second call's blocks: frames 1 and 2 remain (frame 0 never reached them)"
    assert sum(int((f12[k] != f1[k]).any(-1).sum()) for k in later) >= 50, "frame 2 must matter beyond the cut"


def test_remove_twice_underflows_and_leaves_those_voxels_alone():
    scn = RC.scenarios()["remove_twice"]
    once, _, u1 = RC.run(scn, calls=2)
    ref, after, under = RC.reference_of("remove_twice")
    assert u1[1] == 0 and under[2] > 1000 and ref.status & RR.UNDERFLOW and ref.n_underflow == under[2] == len(ref.underflowed)
    print("underflowed voxels:", under[2])
    for k, l in ref.underflowed:
        assert (ref.blocks[k][l] == once.blocks[k][l]).all()
    assert all((v >= 0).all() for v in ref.blocks.values()), "no sum ever wraps"


def test_split_calls_agree_with_one_call_on_the_blocks_that_existed():
    """the moved frames in two calls: the blocks claimed before the calls receive every frame's new side either way; a block the second call claims
    has not seen the first call's frames (INTEGRATION's own rule for later calls)"""
    one, a1, _ = RC.reference_of("move_all/scene")
    two, a2, _ = RC.reference_of("split_calls")
    assert a1[0] == a2[0] and set(one.blocks) == set(two.blocks)
    old = list(one.blocks)[:a1[0]]
    assert all((one.blocks[k] == two.blocks[k]).all() for k in old)


def test_moving_back_restores_the_sums():
    ref, after, under = RC.reference_of("move_back")
    orig = TC.reference_of("scene")
    assert under == [0, 0, 0] and after[2] == after[1] > after[0] == len(orig.blocks)
    assert _blocks_equal_on(ref, orig) == 0
    # the blocks the move claimed: the move's own sums are taken out again (the reach of the moved frames covers them) and the frames, back at their
    # first poses, now reach them
    scn = RC.scenarios()["move_back"]
    late = list(ref.blocks)[after[0]:]
    want = RC.sums_on(scn, late, range(4))
    assert all((ref.blocks[k] == want[k]).all() for k in late)


def test_many_frames_span_the_mask_words():
    for n in RC.MANY:
        scn = RC.scenarios()["many_frames/%d" % n]
        ref, after, under = RC.reference_of("many_frames/%d" % n)
        ids = scn["case"]["map_id"]
        assert (n + 63) // 64 == {65: 2, 129: 3}[n] and ids[n - 1] >= 0 and np.isfinite(scn["case"]["T"][n - 1]).all(), "the last word holds a live frame"
        assert under[1] == 0 and {k[0] for k in ref.blocks} == {0, 3}
