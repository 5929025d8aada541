"""Inputs of the surface map's scale tests (tests/test_tsdf_scale_cases.py on the CPU, tests/test_gpu_tsdf_scale.py on the device): the sizes
KeyframePipeline.surface_map() runs at and tests/tsdf_cases.py / tests/tsdf_mesh_cases.py (at most four frames, 27 blocks, weights to 10) stay below --
calls of more than 64 and more than 256 frames, block lists longer than the 4096 workgroups that walk them, weights up to the limit 2^20.  The
yardsticks are tests/tsdf_ref.py and tests/tsdf_mesh_ref.py, unchanged; the CPU test holds every case to the conditions that make it mean something.

A reference "with loaded blocks" is a TsdfRef whose `blocks` are preset (int64) before integrate(): with_blocks()."""
import functools

import numpy as np

import tsdf_cases as TC
import tsdf_mesh_cases as MC
import tsdf_ref as TR

GRID = 4096            # kTsdfGrid: the workgroups of every kernel that walks the block list
MAX_W = TR.MAX_W       # 2^20
LOG2_BLOCKS = 13       # the pool of the long lists: 8192 slots of 8 KiB
PAD_MAP = 9
FRAME_COUNTS = (64, 65, 130, 260)
MAX_BATCH = 260        # the context of the many-frame calls: five frame-mask words per block


# ------------------------------------------------------------------------------------------------------------------------ A. many frames
def planted(n):
    """the frames of many_frames(n) whose pose is not finite.  In the long calls they lie beyond the first mask word, in the 260-frame call one also
    beyond the frame table's first trip of 256 lanes.  64 frames have no frame beyond the first word, and of 65 frames the second word holds frame 64
    alone, which must stay finite for that word to matter: there the pose lies below 64."""
    return [37] if n < 128 else [70] if n < 260 else [70, 258]


def away(b):
    """every fifth frame looks the other way"""
    return b % 5 == 2


def _map_of(b):
    return -1 if b % 23 == 11 else 3 if b % 7 == 6 else 0


@functools.lru_cache(maxsize=None)
def many_frames(n, seed=9):
    """n frames 37 x 48 around the three poses of synth.trajectory(3, 9), so that every frame of a map meets the same few blocks and every word of
    64 frames adds to every block; every fifth frame turned half round about the camera's y axis (its blocks lie behind the others, and the cull
    drops each group's pairs with the other's blocks); map 0, every seventh frame map 3, a few frames without a map; planted(n) not finite"""
    synth = TC._synth()
    rng = np.random.default_rng(seed)
    scene = synth.Scene(seed=9, n_walls=14, z_far=30.0)
    base = [np.asarray(t, np.float64) for t in synth.trajectory(3, 9)]
    cam, w, h = TC.CAM_NARROW, 37, TC.H
    half = synth.rot_y(np.pi)
    T = np.zeros((n, 7))
    disp = np.zeros((n, h, w), np.float32)
    gray = np.zeros((n, h, TC.PITCH), np.uint8)
    for b in range(n):
        t = base[b % 3]
        if away(b):
            t = synth.se3_from_Rt(half @ synth.R_from_quat(t[:4]), half @ t[4:])
        T[b] = synth.perturb_pose(t, rng, 0.02)
        img, depth = scene.render(T[b], w=w, h=h, cam=cam)
        with np.errstate(divide="ignore"):
            disp[b] = (cam[0] * cam[4] / depth).astype(np.float32)
        gray[b, :, :w] = img
    map_id = np.array([_map_of(b) for b in range(n)], np.int32)
    for k, b in enumerate(planted(n)):
        assert map_id[b] >= 0
        T[b, (5, 1)[k % 2]] = (np.nan, np.inf)[k % 2]
    case = TC._case("many_%d" % n, cam, disp, gray, T, 0.25, 2, 2.0, 10.0, step=2, map_id=map_id)
    for a in (disp, gray, T, map_id):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def many_reference(n):
    """the restatement of the one call of many_frames(n), computed once and shared: do not change it"""
    return TC.reference(many_frames(n))


def pairs_visited(case, ref):
    """what n_pairs_visited must be after one call: over the maps, (blocks of the map) x (frames of the map with a finite pose)"""
    fin = [b for b in range(len(case["T"])) if case["map_id"][b] >= 0 and np.isfinite(case["T"][b]).all()]
    return sum(sum(k[0] == m for k in ref.blocks) * sum(case["map_id"][b] == m for b in fin) for m in {int(case["map_id"][b]) for b in fin})


def min_weights(n):
    """the thresholds the many-frame extractions run at: n // 4 leaves no surfel in this scene (the surface lies near z_max, and a frame in three
    sees it), 3 n // 16 is the largest of these that leaves some"""
    return (1, n // 8, 3 * n // 16, n // 4)


def word_permutation(n):
    """a permutation of n frames that moves frames between the words of 64: a fixed shuffle"""
    return np.random.default_rng(130).permutation(n)


# ------------------------------------------------------------------------------------------------------------------------ B. long lists
def with_blocks(ids, voxels, voxel_size, J, cam):
    """a TsdfRef that holds the given raw blocks, as a map does after load_blocks"""
    ref = TR.TsdfRef(voxel_size, J, cam)
    ref.blocks = {tuple(k): v.astype(np.int64) for k, v in zip(np.asarray(ids).tolist(), np.asarray(voxels))}
    return ref


def padding(n):
    """n blocks of map PAD_MAP with no voxel seen, on a lattice of every second block from coordinate 100: next to nothing"""
    i = np.arange(n)
    ids = np.stack([np.full(n, PAD_MAP), 100 + 2 * (i % 17), 100 + 2 * ((i // 17) % 17), 100 + 2 * (i // 289)], 1).astype(np.int32)
    assert n <= 17 ** 3 and len(np.unique(ids, axis=0)) == n
    return ids, np.zeros((n, 512, 4), np.uint32)


def _as_map(ids, m):
    out = np.array(ids, np.int32)
    out[:, 0] = m
    return out


@functools.lru_cache(maxsize=None)
def long_list():
    """the three loads of the long mesh map, in order: noise_holes as map 0 (list positions 0 .. 25), padding up to position GRID - 1, noise_full as
    map 5 from position GRID: workgroup g < 26 walks a noise block, then a second one"""
    c = MC.cases()
    first = (_as_map(c["noise_holes"]["ids"], 0), c["noise_holes"]["voxels"])
    pad = padding(GRID - len(first[0]))
    last = (_as_map(c["noise_full"]["ids"], 5), c["noise_full"]["voxels"])
    return [first, pad, last]


@functools.lru_cache(maxsize=None)
def long_union():
    """(ids, voxels) of the three loads together"""
    parts = long_list()
    ids, vox = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    ids.setflags(write=False); vox.setflags(write=False)
    return ids, vox


@functools.lru_cache(maxsize=None)
def long_mesh(map_id=-1):
    """the yardstick's canonical mesh of the union (its vertices are TsdfRef.extract of the same blocks, which MR.mesh calls), computed once and
    shared: do not change it"""
    import tsdf_mesh_ref as MR
    ids, vox = long_union()
    return MR.mesh(ids, vox, MC.VOXEL_SIZE, 1, map_id)


CULL_WAVES = 4         # tsdf_cull_kernel: one wave per (list entry, word of 64 frames), kVoxelBlock / 64 waves per workgroup, GRID workgroups


@functools.lru_cache(maxsize=None)
def cull_second_trip():
    """what is loaded before many_frames(260) is integrated so that the cull's (entry, word) items outnumber its waves: every second block of the
    call's restatement with no voxel seen (claimed first: list positions 0 .. 22, items of the first trip), then padding up to position GRID + 3.
    The call claims the other blocks behind the padding, where every item is one of the second trip.  A block loaded empty is what the
    allocation would have claimed: the answer is many_reference(260) with the padding next to it.
    -> (the loads, (ids, voxels) of the answer, the list's length after the call)"""
    ref = many_reference(260)
    early = np.array(sorted(ref.blocks)[::2], np.int32)
    pad = padding(GRID + 4 - len(early))
    ids, vox = ref.dump()
    ids, vox = np.concatenate([ids, pad[0]]), np.concatenate([vox, pad[1]])
    order = np.lexsort((ids[:, 3], ids[:, 2], ids[:, 1], ids[:, 0]))
    return [(early, np.zeros((len(early), 512, 4), np.uint32)), pad], (ids[order], vox[order]), len(ids)


SCENE_SPLIT = [[0, 1], [2, 3]]


@functools.lru_cache(maxsize=None)
def scene_pad():
    """the padding blocks loaded between the scene's two calls: with what the first call claims the list then holds GRID + 1 entries, so the blocks
    the second call claims start at position GRID + 1 -- workgroup g walks a block of the first call, then one of the second"""
    return GRID + 1 - len(TC.reference(TC.cases()["scene"], frames=SCENE_SPLIT[0]).blocks)


@functools.lru_cache(maxsize=None)
def scene_padded_reference():
    """the scene of tests/tsdf_cases.py in the two calls SCENE_SPLIT with scene_pad() padding blocks in the map: (the restatement after the first call
    alone, the restatement after both), computed once and shared: do not change them"""
    case = TC.cases()["scene"]
    out = []
    for calls in (SCENE_SPLIT[:1], SCENE_SPLIT):
        ref = with_blocks(*padding(scene_pad()), case["voxel_size"], case["J"], case["cam"])
        out.append(TC.reference(case, ref=ref, calls=calls))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------ C. weights at the limit
@functools.lru_cache(maxsize=None)
def heavy(over=False):
    """the 26 blocks of noise_holes with W uniform in [2^19, 2^20 - 1], Wc = W, Sq = 1024 W + q (W // 2) with q in [-1024, 1024] (num = q (W // 2): Sq
    runs up to 1.5 * 2^30), I = i Wc with i <= 255.  over: one voxel in the middle of a block at W = 2^20."""
    rng = np.random.default_rng(21)
    ids = np.array(MC.cases()["noise_holes"]["ids"], np.int32)
    shape = (len(ids), 512)
    W = rng.integers(1 << 19, 1 << 20, shape)
    q = rng.integers(-1024, 1025, shape)
    inten = rng.integers(0, 256, shape)
    W[3, 100], q[3, 100] = MAX_W - 1, 1024      # the largest weight that is good, under the largest sum
    W[4, 200], q[4, 200] = 1 << 19, -1024
    if over:
        W[7, (3 << 6) | (4 << 3) | 2] = MAX_W
    Sq = 1024 * W + q * (W // 2)
    assert Sq.min() >= 0 and Sq.max() < 2 ** 32 and (inten * W).max() < 2 ** 32
    vox = np.stack([W, Sq, W, inten * W], -1).astype(np.uint32)
    ids.setflags(write=False); vox.setflags(write=False)
    return dict(ids=ids, voxels=vox, voxel_size=MC.VOXEL_SIZE)


@functools.lru_cache(maxsize=None)
def heavy_mesh(over=False):
    import tsdf_mesh_ref as MR
    c = heavy(over)
    return MR.mesh(c["ids"], c["voxels"], c["voxel_size"])


def surfels_and_status(ids, voxels, voxel_size, min_weight=1):
    """(TsdfRef.extract of raw blocks, the status the extraction leaves)"""
    ref = with_blocks(ids, voxels, voxel_size, 1, (1.0, 1.0, 0.0, 0.0, 1.0))
    s = ref.extract(min_weight=min_weight)
    return s, ref.status


LIMIT_W = MAX_W - 2


@functools.lru_cache(maxsize=None)
def scene_at_the_limit():
    """the scene's first two frames, every seen voxel scaled to weight 2^20 - 2 (each of its views counted (2^20 - 2) // W times: W, Sq, Wc and I
    scale alike, D and the intensity stay), then the other two frames on top: (loaded ids, loaded voxels, the restatement after frames [2, 3])"""
    case = TC.cases()["scene"]
    ids, vox = TC.reference(case, frames=[0, 1]).dump()
    vox = vox.astype(np.int64)
    W = vox[..., 0]
    k = np.where(W > 0, LIMIT_W // np.maximum(W, 1), 1)
    assert set(np.unique(W).tolist()) <= {0, 1, 2}, "two views at the most: k W is 2^20 - 2 exactly"
    vox = vox * k[..., None]
    assert vox.max() < 2 ** 32 and (vox[..., 0][W > 0] == LIMIT_W).all()
    ref = with_blocks(ids, vox, case["voxel_size"], case["J"], case["cam"])
    TC.reference(case, frames=[2, 3], ref=ref)
    return ids, vox.astype(np.uint32), ref


# ------------------------------------------------------------------------------------------------------------------------ D. regrowth
@functools.lru_cache(maxsize=None)
def regrown():
    """two_maps, then noise_full loaded over it (the eight blocks both hold take noise_full's voxels): (ids, voxels) of the union"""
    c = MC.cases()
    blocks = {tuple(k): v for k, v in zip(c["two_maps"]["ids"].tolist(), c["two_maps"]["voxels"])}
    blocks.update({tuple(k): v for k, v in zip(c["noise_full"]["ids"].tolist(), c["noise_full"]["voxels"])})
    keys = sorted(blocks)
    return np.array(keys, np.int32), np.stack([blocks[k] for k in keys])


# ------------------------------------------------------------------------------------------------------------------------ E. small paths
@functools.lru_cache(maxsize=None)
def small(name):
    """narrow, random, or random_step1: random with every pixel allocating (step 1 is where the allocation loads 16-byte rows or, off that alignment,
    pixel by pixel)"""
    return dict(TC.cases()["random"], name=name, step=1) if name == "random_step1" else TC.cases()[name]


@functools.lru_cache(maxsize=None)
def small_reference(name, with_gray=True):
    """computed once and shared: do not change it"""
    case = small(name)
    if with_gray and name in TC.cases():
        return TC.reference_of(name)
    ref = TR.TsdfRef(case["voxel_size"], case["J"], case["cam"])
    ref.integrate(case["disp"], case["gray"] if with_gray else None, case["T"], case["map_id"], case["z_min"], case["z_max"], case["step"])
    return ref
