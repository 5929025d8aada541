"""Inputs of the re-integration tests (tests/test_tsdf_reintegrate_ref.py on the CPU, tests/test_gpu_tsdf_reintegrate.py on the device): scenarios
over the cases of tests/tsdf_cases.py (160 x 48 and 37 x 48 images, 2-4 frames) and the many-frame calls of tests/tsdf_scale_cases.py.

A scenario is a case (camera, images, gates) and a list of calls.  A call is
    dict(kind="integrate", frames, T, map_id)                               vslam_tsdf_integrate_dev
    dict(kind="reintegrate", frames, T_old, T_new, map_id, reach)            vslam_tsdf_reintegrate_dev
with `frames` the indices into the case's images (a frame may be listed more than once), and each entry of `reach` either a number or
("after", k): the block count after call k of the scenario, which is the reach of the frames call k integrated.  New poses are
synth.perturb_pose of the old ones with fixed seeds; a switched-off side is an all-NaN pose."""
import functools

import numpy as np

import tsdf_cases as TC
import tsdf_reintegrate_ref as RR
import tsdf_scale_cases as SC

SIGMA = 0.02            # the pose noise of tests/tsdf_cases.py's own trajectories
MANY = (65, 129)        # frames of the many-frame scenarios: two and three mask words
NAN7 = np.full(7, np.nan)
# The seed of each move_all scenario's new poses.  With a thinned allocation (step > 1) the fresh map at the new poses lacks blocks that hold part of the
# surface, and a block only the OLD poses claimed may then hold a crossing the fresh map has no block for: the sums agree on every block of the fresh
# map whatever the seed, the surfel lists only where no such block does.  j8_step3's seed is one of those (2 of the 12 seeds 101 .. 112 are).
MOVE_SEEDS = dict(below_zero_j1=100, j8_step3=106, narrow=102, random=103, scene=104)


def perturbed(T, seed, sigma=SIGMA):
    """every pose of T (n, 7) moved by synth.perturb_pose; a pose that is not finite stays as it is"""
    synth = TC._synth()
    rng = np.random.default_rng(seed)
    return np.stack([synth.perturb_pose(np.asarray(t, np.float64), rng, sigma) if np.isfinite(t).all() else np.array(t, np.float64) for t in T])


def _integrate(case, frames, map_id=None):
    frames = list(frames)
    return dict(kind="integrate", frames=frames, T=case["T"][frames], map_id=case["map_id"][frames] if map_id is None else np.asarray(map_id, np.int32))


def _reint(case, frames, T_old, T_new, reach, map_id=None):
    frames = list(frames)
    n = len(frames)
    T_old = np.tile(NAN7, (n, 1)) if T_old is None else np.asarray(T_old, np.float64)
    T_new = np.tile(NAN7, (n, 1)) if T_new is None else np.asarray(T_new, np.float64)
    reach = list(reach) if isinstance(reach, list) else [reach] * n
    assert len(T_old) == len(T_new) == len(reach) == n
    return dict(kind="reintegrate", frames=frames, T_old=T_old, T_new=T_new, reach=reach,
                map_id=case["map_id"][frames] if map_id is None else np.asarray(map_id, np.int32))


def _all(case):
    return list(range(len(case["disp"])))


@functools.lru_cache(maxsize=None)
def scenarios():
    """name -> dict(case, calls)"""
    out = {}
    cases = TC.cases()
    for name in sorted(cases):
        c = cases[name]
        out["move_all/" + name] = dict(case=c, calls=[_integrate(c, _all(c)), _reint(c, _all(c), c["T"], perturbed(c["T"], MOVE_SEEDS[name]), ("after", 0))])
    c = cases["scene"]
    T, T2 = c["T"], perturbed(c["T"], MOVE_SEEDS["scene"])
    out["remove_all"] = dict(case=c, calls=[_integrate(c, _all(c)), _reint(c, _all(c), T, None, ("after", 0))])
    out["two_calls_remove_first"] = dict(case=c, calls=[_integrate(c, [0]), _integrate(c, [1, 2, 3]), _reint(c, [0], T[[0]], None, ("after", 0))])
    # one call: a moved frame, a removed frame, a frame whose poses are equal, a frame without a map, a plain addition, a moved frame of the other map
    ids = np.array([0, 0, 1, 1], np.int32)
    fr = [0, 1, 2, 3, 0, 3]
    Ta = perturbed(T[[0]], 131)[0]
    out["mixed"] = dict(case=c, calls=[
        _integrate(c, _all(c), map_id=ids),
        _reint(c, fr, T_old=np.stack([T[0], T[1], T[2], T[3], NAN7, T[3]]), T_new=np.stack([T2[0], NAN7, T[2], T2[3], Ta, T2[3]]), reach=("after", 0),
               map_id=[0, 0, 1, -1, 1, 1])])
    # removals with reach 0 (nothing is taken out), a cut in the middle of the list (the first call's count) and a reach above the list's length
    out["reach_edges"] = dict(case=c, calls=[_integrate(c, [0]), _integrate(c, [1, 2, 3]), _reint(c, [1, 2, 3], T[[1, 2, 3]], None, [0, ("after", 0), 10 ** 6])])
    out["remove_twice"] = dict(case=c, calls=[_integrate(c, _all(c)), _reint(c, [0, 1], T[[0, 1]], None, ("after", 0)), _reint(c, [0, 1], T[[0, 1]], None, ("after", 0))])
    # the moved frames in two calls, the reach updated between them, and moved back with the reach each frame then has
    out["split_calls"] = dict(case=c, calls=[_integrate(c, _all(c)), _reint(c, [0, 1], T[[0, 1]], T2[[0, 1]], ("after", 0)), _reint(c, [2, 3], T[[2, 3]], T2[[2, 3]], ("after", 0))])
    out["move_back"] = dict(case=c, calls=[_integrate(c, _all(c)), _reint(c, _all(c), T, T2, ("after", 0)), _reint(c, _all(c), T2, T, ("after", 1))])
    for n in MANY:
        m = SC.many_frames(n)
        out["many_frames/%d" % n] = dict(case=m, calls=[_integrate(m, _all(m)), _reint(m, _all(m), m["T"], perturbed(m["T"], 200 + n), ("after", 0))])
    return out


def resolve(reach, after):
    """the numbers of a call's `reach`, given the block counts after the scenario's earlier calls"""
    return np.array([after[r[1]] if isinstance(r, tuple) else r for r in reach], np.int64)


def run(scn, calls=None, ignore_reach=False):
    """the yardstick fed the scenario (or its first `calls` calls) -> (ref, the block count after each call, the underflowed voxels of each call).
    ignore_reach: every reach replaced by the block count at the time of the call, as a kernel that ignores reach would behave"""
    c = scn["case"]
    ref = RR.TsdfReintRef(c["voxel_size"], c["J"], c["cam"])
    after, under = [], []
    for call in scn["calls"][:calls]:
        fr = call["frames"]
        if call["kind"] == "integrate":
            ref.integrate(c["disp"][fr], c["gray"][fr], call["T"], call["map_id"], c["z_min"], c["z_max"], c["step"])
            under.append(0)
        else:
            reach = np.full(len(fr), 10 ** 9) if ignore_reach else resolve(call["reach"], after)
            under.append(ref.reintegrate(c["disp"][fr], c["gray"][fr], call["T_old"], call["T_new"], call["map_id"], reach, c["z_min"], c["z_max"], c["step"]))
        after.append(ref.reach())
    return ref, after, under


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """run() of a whole scenario, computed once and shared: do not change it"""
    return run(scenarios()[name])


def fresh(scn, T, frames=None, map_id=None):
    """a new map with the scenario's frames (or `frames`) integrated at the poses T in one call"""
    c = scn["case"]
    fr = _all(c) if frames is None else list(frames)
    ref = RR.TsdfReintRef(c["voxel_size"], c["J"], c["cam"])
    ref.integrate(c["disp"][fr], c["gray"][fr], np.asarray(T)[fr], c["map_id"][fr] if map_id is None else map_id, c["z_min"], c["z_max"], c["step"])
    return ref


def sums_on(scn, keys, frames):
    """what the scenario's `frames`, at the case's poses, add to the blocks `keys` (whether or not their own allocation would claim them): key -> sums"""
    c = scn["case"]
    fr = list(frames)
    ref = RR.TsdfReintRef(c["voxel_size"], c["J"], c["cam"])
    ref.blocks = {k: np.zeros((512, 4), np.int64) for k in keys}
    ref.integrate(c["disp"][fr], c["gray"][fr], c["T"][fr], c["map_id"][fr], c["z_min"], c["z_max"], c["step"])
    return {k: ref.blocks[k] for k in keys}
