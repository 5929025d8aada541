"""Structured, tie-dense inputs for the ORB / ANMS / SGBM parity tests (tests/test_structured_inputs.py on the CPU, tests/test_gpu_ties.py on
the device, the `orb_ties` and `sgbm_periodic` kinds of tests/fuzz_parity.py).  Plain numpy, seeded, nothing on disk; the helpers that count ties
or capacities take the oracle module as their argument `O`.

Noise images -- everything the parity suite used before -- never make two keypoints share a response, never put a pyramid level above its
quota and give ANMS one tied radius at most, so none of the tie rules of the selection (ties at a retainBest cut are kept), of ANMS (stable
order by (response, input index), every radius >= the num-th largest is kept) or of SGBM (the first minimum over d wins) decides anything.
Repeating structure does: a tiled patch repeats every corner with the same FAST score, Harris response and neighbourhood, a mirrored image
pairs them, a checkerboard's corners are all alike, a horizontally periodic stereo pair has exact cost ties at d, d + p, d + 2p.

ORB_CASES is the table of the ORB cases with their sizes and the tie counts the CPU oracle gives for them (`oracle` columns) next to the floors
tests/test_structured_inputs.py asserts (`floor` = half of the oracle's figure, rounded down): a floor is a condition on the INPUT -- that it
still has the ties it is named for -- not a measurement of the code under test.  tests/test_structured_inputs.py::test_table_figures_are_current
fails with the fresh numbers if a generator or the oracle changes them."""
import numpy as np

# cv::KeyPoint as the C-ABI and the oracle lay it out (28 bytes)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

KITTI = (376, 1241)
ODD = (257, 333)
WIDE = (200, 1324)


# ------------------------------------------------------------------ image generators, all (h, w) uint8
def tiled_patch(h, w, t, seed=0, cell=2):
    """a random t x t patch (uniform grey levels in cell x cell blocks) repeated over the image: every corner recurs with period t in both
    directions.  (cell = 1, white noise, has more FAST corners than the device's per-level corner lists hold.)"""
    g = np.random.default_rng(seed).integers(0, 256, (t // cell + 1, t // cell + 1), dtype=np.uint8)
    p = np.kron(g, np.ones((cell, cell), np.uint8))[:t, :t]
    return np.ascontiguousarray(np.tile(p, (h // t + 1, w // t + 1))[:h, :w])


def blocky_noise(h, w, seed=0, cells=((9, 110), (3, 90))):
    """blocky uniform noise at two scales (no smooth term: grey levels recur)"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128.0)
    for cell, amp in cells:
        g = rng.uniform(-0.5, 0.5, (h // cell + 2, w // cell + 2))
        img += amp * np.kron(g, np.ones((cell, cell)))[:h, :w]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def mirrored_noise(h, w, seed=0):
    """blocky noise whose left half is mirrored onto the right: every corner has a twin (same score, same response, angle reflected)"""
    img = blocky_noise(h, w, seed)
    half = w // 2
    img[:, w - half:] = img[:, :half][:, ::-1]
    return img


def checkerboard(h, w, s, lo=40, hi=215):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // s) + (xx // s)) % 2 == 0, lo, hi).astype(np.uint8)


def quantised_blocks(h, w, levels=2, block=4, seed=0):
    """block x block cells, each at one of `levels` evenly spaced grey levels"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, levels, (h // block + 1, w // block + 1))
    v = np.rint(np.linspace(30, 225, levels)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(v[g], np.ones((block, block), np.uint8))[:h, :w])


def binary_noise(h, w, seed=0, block=3):
    """two grey levels in block x block cells (per-pixel salt and pepper overflows the device's FAST corner lists: that input has its own
    test, test_corner_capacity_overflow_is_an_error)"""
    return quantised_blocks(h, w, 2, block, seed)


def step_edges(h, w, period=24, lo=60, hi=190):
    """vertical step edges every period / 2 columns: straight edges, no FAST corner anywhere"""
    xx = np.arange(w)
    return np.ascontiguousarray(np.broadcast_to(np.where((xx // (period // 2)) % 2 == 0, lo, hi).astype(np.uint8), (h, w)))


def linear_ramp(h, w, gx=1, gy=0):
    """grey = 128 + (gx x + gy y) / 4 around the centre, clipped: constant gradient"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(128 + (gx * (xx - w // 2) + gy * (yy - h // 2)) // 4, 0, 255).astype(np.uint8)


def blob_lattice(h, w, pitch=36, bg=20, amps=(70, 110, 160, 230), half=2):
    """a constant image with identical square blobs ((2 half + 1)^2 pixels, the centre pixel 20 grey levels above the rest so that it is the
    strict FAST-score maximum) on a square lattice; the blob at lattice node (i, j) has the amplitude amps[(i + 2 j) % len(amps)].  Blobs of one
    amplitude give identical keypoints (equal response: the stable sort decides their order), and the nearest stronger blob of every node of one class lies at the same offset:
    whole classes share one suppression radius."""
    img = np.full((h, w), bg, np.uint8)
    for j, y in enumerate(range(40, h - 40, pitch)):
        for i, x in enumerate(range(40, w - 40, pitch)):
            img[y - half:y + half + 1, x - half:x + half + 1] = amps[(i + 2 * j) % len(amps)]
            img[y, x] = amps[(i + 2 * j) % len(amps)] + 20
    return img


GENERATORS = dict(tiled=tiled_patch, mirror=mirrored_noise, checker=checkerboard, quant=quantised_blocks, binary=binary_noise, steps=step_edges,
                  ramp=linear_ramp, blobs=blob_lattice, blocky=blocky_noise)


def make(case):
    """the image of one ORB_CASES / OVERFLOW_CASES row"""
    h, w = case["size"]
    return GENERATORS[case["gen"]](h, w, **case["args"])


# ------------------------------------------------------------------ SGBM
def periodic_pair(period, shift, noise=0, w=385, h=120, seed=4):
    """(left, right) cut from a texture of horizontal period `period` (uniform grey levels, every row its own): left(x) == right(x - shift), and
    just as well right(x - shift - k period): the matching cost has exact ties at d = shift mod period + k period, and "the first minimum over
    d wins" alone says that every evaluated pixel comes out as shift mod period.  noise: +- that many grey levels, uniform, added to the right
    image (then the ties are near-ties the uniqueness and left-right checks judge).

    Every row of the texture is a palindrome (tex[i] == tex[-i mod period]), i.e. mirror-symmetric about the columns 0 and period / 2 (mod
    period).  The winner is refined to 1/16 pixel by a parabola through the summed costs at d - 1 and d + 1; inside the image those two sums
    run over the same pairs of neighbouring columns except one at each end of the 9-column window and the parabola's peak stays at d, but the
    window is clamped at the first evaluated column (96) and at the last one (w - 1), and a generic texture moves the peak there by up to
    3/16.  With 96 and w - 1 both multiples of period / 2 the clamped windows are symmetric too.  KNOWN_ANSWER_SIZES are such sizes.  What is
    left is a pixel or two per image where the end terms alone shift the peak by 1/16: the known-answer tests use the default seed, for
    which the oracle has none at any of their sizes and periods, and check the whole-pixel winner for other seeds."""
    rng = np.random.default_rng(seed)
    i = np.arange(period)
    row = rng.integers(0, 256, (h, period), dtype=np.uint8)[:, np.minimum(i, (period - i) % period)]
    tex = np.tile(row, (1, (w + shift) // period + 2))
    left = np.ascontiguousarray(tex[:, :w]); right = np.ascontiguousarray(tex[:, shift:shift + w])
    if noise:
        right = np.clip(right.astype(int) + rng.integers(-noise, noise + 1, right.shape), 0, 255).astype(np.uint8)
    return left, right


NUM_DISP = 96
# (w, h) with w - 1 a multiple of 96 (= of period / 2 for the periods 24, 32, 48, 64)
KNOWN_ANSWER_SIZES = [(385, 120), (481, 77)]
# a KITTI-sized pair: 1240 and 96 share the factor 8, so the period whose clamped windows are symmetric is 16 (ties at d, d + 16, ..., six of them)
KITTI_PERIODIC = dict(period=16, w=1241, h=376)

# noise-free pairs: shift mod period is 0, small and > period / 2 for every period; every evaluated pixel (x >= 96) must come out as shift mod period
SGBM_CLEAN = [dict(period=24, shift=0), dict(period=24, shift=5), dict(period=24, shift=67),      # 67 mod 24 = 19
              dict(period=32, shift=5), dict(period=32, shift=64), dict(period=32, shift=93),     # 0, 29
              dict(period=48, shift=40), dict(period=48, shift=51), dict(period=48, shift=48),    # 40, 3, 0
              dict(period=64, shift=70), dict(period=64, shift=45), dict(period=64, shift=0)]     # 6, 45
# noisy pairs (385 x 120, default seed): `winners` = disparities of ONE residue class that must each hold at least `floor` of the valid pixels;
# `oracle` = the share the CPU oracle gives them, floor = half of it
SGBM_NOISY = [dict(period=32, shift=5, noise=3, winners={5: dict(oracle=0.2691, floor=0.1345), 37: dict(oracle=0.3299, floor=0.1649), 69: dict(oracle=0.4011, floor=0.2005)}),
              dict(period=64, shift=70, noise=2, winners={6: dict(oracle=0.3915, floor=0.1957), 70: dict(oracle=0.6076, floor=0.3038)}),
              dict(period=24, shift=19, noise=3, winners={19: dict(oracle=0.2472, floor=0.1236), 43: dict(oracle=0.1302, floor=0.0651), 67: dict(oracle=0.1677, floor=0.0838),
                                                         91: dict(oracle=0.4542, floor=0.2271)}),
              dict(period=48, shift=40, noise=4, winners={40: dict(oracle=0.5634, floor=0.2817), 88: dict(oracle=0.4364, floor=0.2182)})]


def sgbm_winner_shares(disp16):
    """{disparity in pixels: share of the valid pixels} of a CV_16S map, whole-pixel disparities only"""
    v = disp16[disp16 >= 0]
    whole = v[v % 16 == 0] // 16
    d, n = np.unique(whole, return_counts=True)
    return {int(k): float(c) / max(len(v), 1) for k, c in zip(d, n)}


# ------------------------------------------------------------------ what the oracle says about a case
def quotas(O, size, nfeatures):
    h, w = size
    return np.array(O.orb_layout(w, h, nfeatures)["nfeat"])


def tie_figures(O, img, nfeatures, nums=(500, 1500)):
    """the tie counts of one image: duplicate responses, keypoints above the level quotas, ANMS output beyond num, exact-zero angles"""
    kps = O.orb_detect(img, nfeatures)
    q = quotas(O, img.shape, nfeatures)
    per = np.bincount(kps["octave"], minlength=8)
    fig = dict(n=len(kps), dup=int(len(kps) - len(np.unique(kps["response"]))), over=int(np.maximum(per - q, 0).sum()), levels_over=int((per > q).sum()),
               angle0=int((kps["angle"] == 0).sum()))
    for num in nums:
        fig["anms%d" % num] = int(len(O.anms(kps, num)) - num) if len(kps) >= num else 0
    return fig


# Device capacities (stereo-visual-slam_amd/csrc/orb_kernels.hip): FAST corner list of a level = area / 16 rounded up to 256, candidates of a
# level after the FAST-score cut = 4096, selected keypoints of a level = 1024, keypoints of an image entering ANMS = 3328, output = kp_capacity
ST_CORNER, ST_CAND, ST_SEL, ST_ANMS, ST_OUT = 1, 2, 4, 8, 16
CAND_CAP, SEL_CAP, ANMS_CAP = 4096, 1024, 3328


def device_capacity_bits(O, img, nfeatures, anms_num, kp_capacity=4096, describe=True, fast_threshold=20):
    """the ORB status bits the device must raise for this image, from the oracle's counts stage by stage: (bits, counts).  A stage behind an
    overflowing one sees a truncated list whose content is not defined; its bit is predicted from the truncated COUNT where that is defined
    (the selection truncates a level to 1024) and left out of `bits` but named in counts["unknown"] where it is not."""
    h, w = img.shape
    L = O.orb_layout(w, h, nfeatures)
    lv = O.build_pyramid(img, 8, nfeatures)
    bits = 0; unknown = 0
    corners, cands = [], []
    for l in range(8):
        c = O.fast9_16(lv[l], fast_threshold, True)
        c = c[(c["x"] >= 31) & (c["x"] < L["w"][l] - 31) & (c["y"] >= 31) & (c["y"] < L["h"][l] - 31)]
        corners.append(len(c)); cands.append(len(O.retain_best(c, 2 * L["nfeat"][l])))
        if len(c) > ((L["w"][l] * L["h"][l] // 16 + 255) & ~255):
            bits |= ST_CORNER; unknown |= ST_CAND | ST_SEL | ST_ANMS | ST_OUT
        if cands[-1] > CAND_CAP:
            bits |= ST_CAND; unknown |= ST_SEL | ST_ANMS | ST_OUT
    kps = O.orb_detect(img, nfeatures, cap=1 << 16, fast_threshold=fast_threshold)
    sel = np.bincount(kps["octave"], minlength=8)
    if not unknown & ST_SEL and (sel > SEL_CAP).any():
        bits |= ST_SEL; unknown |= ST_OUT
    n_in = int(np.minimum(sel, SEL_CAP).sum())
    if not unknown & ST_ANMS and n_in > ANMS_CAP:
        bits |= ST_ANMS; unknown |= ST_OUT
    n_out = None
    if min(n_in, ANMS_CAP) <= kp_capacity:   # whatever a truncated list holds, no more than that many keypoints leave ANMS
        unknown &= ~ST_OUT
    if not bits:
        k = O.anms(kps, anms_num) if anms_num > 0 else kps
        if describe:
            k = k[(k["x"] >= 31) & (k["x"] < w - 31) & (k["y"] >= 31) & (k["y"] < h - 31)]
        n_out = len(k)
        if n_out > kp_capacity:
            bits |= ST_OUT
    return bits, dict(corners=corners, cands=cands, sel=sel.tolist(), anms_in=n_in, out=n_out, unknown=unknown & ~bits)


# ------------------------------------------------------------------ the ORB cases
# oracle: tie_figures() of the CPU oracle for the committed generator arguments; floor: what test_structured_inputs asserts (oracle // 2).
#   dup = keypoints whose response another keypoint has too; over = keypoints above their level's quota (ties kept at a retainBest cut);
#   anms500 / anms1500 = len(anms(kps, num)) - num (ties kept at the num-th radius); angle0 = keypoints with angle == 0 exactly
ORB_CASES = [
    dict(name='tile20', gen='tiled', args={'t': 20}, size=KITTI, nfeatures=3000,
         oracle={'n': 3218, 'dup': 869, 'over': 218, 'levels_over': 1, 'angle0': 0, 'anms500': 370, 'anms1500': 0},
         floor={'dup': 434, 'over': 109, 'anms500': 185}),
    dict(name='tile32', gen='tiled', args={'t': 32}, size=KITTI, nfeatures=3000,
         oracle={'n': 3078, 'dup': 728, 'over': 78, 'levels_over': 1, 'angle0': 0, 'anms500': 230, 'anms1500': 0},
         floor={'dup': 364, 'over': 39, 'anms500': 115}),
    dict(name='tile60', gen='tiled', args={'t': 60, 'cell': 3}, size=KITTI, nfeatures=3000,
         oracle={'n': 3068, 'dup': 713, 'over': 68, 'levels_over': 1, 'angle0': 0, 'anms500': 5, 'anms1500': 0},
         floor={'dup': 356, 'over': 34, 'anms500': 2}),
    dict(name='tile97', gen='tiled', args={'t': 97}, size=KITTI, nfeatures=3000,
         oracle={'n': 3015, 'dup': 650, 'over': 15, 'levels_over': 1, 'angle0': 0, 'anms500': 0, 'anms1500': 10},
         floor={'dup': 325, 'over': 7, 'anms1500': 5}),
    dict(name='mirror', gen='mirror', args={'seed': 0}, size=KITTI, nfeatures=3000,
         oracle={'n': 3003, 'dup': 1408, 'over': 3, 'levels_over': 3, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 704, 'over': 1, 'levels_over': 1}),
    dict(name='checker8', gen='checker', args={'s': 8}, size=KITTI, nfeatures=3000,
         oracle={'n': 2116, 'dup': 922, 'over': 2, 'levels_over': 2, 'angle0': 59, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 461, 'over': 1, 'levels_over': 1, 'angle0': 29}),
    dict(name='checker31', gen='checker', args={'s': 31}, size=KITTI, nfeatures=3000,
         oracle={'n': 1683, 'dup': 100, 'over': 0, 'levels_over': 0, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 50}),
    dict(name='binary3', gen='binary', args={'block': 3}, size=KITTI, nfeatures=3000,
         oracle={'n': 3101, 'dup': 749, 'over': 101, 'levels_over': 1, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 374, 'over': 50}),
    dict(name='blobs', gen='blobs', args={'half': 1}, size=KITTI, nfeatures=3000,
         oracle={'n': 1632, 'dup': 297, 'over': 0, 'levels_over': 0, 'angle0': 301, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 148, 'angle0': 150}),
    dict(name='steps', gen='steps', args={}, size=KITTI, nfeatures=3000,
         oracle={'n': 0, 'dup': 0, 'over': 0, 'levels_over': 0, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={}),
    dict(name='ramp', gen='ramp', args={}, size=KITTI, nfeatures=3000,
         oracle={'n': 0, 'dup': 0, 'over': 0, 'levels_over': 0, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={}),
    dict(name='tile40_wide', gen='tiled', args={'t': 40}, size=WIDE, nfeatures=3000,
         oracle={'n': 2728, 'dup': 690, 'over': 44, 'levels_over': 1, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 345, 'over': 22}),
    dict(name='quant3_wide', gen='quant', args={'levels': 3, 'block': 5}, size=WIDE, nfeatures=3000,
         oracle={'n': 2655, 'dup': 377, 'over': 0, 'levels_over': 0, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 188}),
    dict(name='tile20_odd', gen='tiled', args={'t': 20}, size=ODD, nfeatures=1000,
         oracle={'n': 1014, 'dup': 268, 'over': 53, 'levels_over': 1, 'angle0': 0, 'anms500': 2, 'anms1500': 0},
         floor={'dup': 134, 'over': 26, 'anms500': 1}),
    dict(name='mirror_odd', gen='mirror', args={'seed': 1}, size=ODD, nfeatures=1000,
         oracle={'n': 952, 'dup': 465, 'over': 6, 'levels_over': 6, 'angle0': 0, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 232, 'over': 3, 'levels_over': 3}),
    dict(name='blobs_odd', gen='blobs', args={'half': 1, 'pitch': 30}, size=ODD, nfeatures=1000,
         oracle={'n': 244, 'dup': 50, 'over': 0, 'levels_over': 0, 'angle0': 54, 'anms500': 0, 'anms1500': 0},
         floor={'dup': 25, 'angle0': 27}),
]
CASE = {c["name"]: c for c in ORB_CASES}

# Inputs that must end in the capacity error on the device, never in a truncated keypoint set.  bits = the status bits that device_capacity_bits()
# derives from the oracle's counts (tests/test_structured_inputs.py checks that it does); may = bits a stage behind a truncated list may add.
#   tile12: 2548 tied keypoints on level 0 > 1024; level 7 nearly empty, so the truncated total (3196) stays under the ANMS capacity
#   tile16: 1406 on level 0, and 1024 + the seven full quotas = 3372 > 3328
#   blocky3600: orb_nfeatures 3600 -> quotas 782, 652, ... all under 1024, together 3600 > 3328
#   binary2: 6274 level-0 corners share ONE FAST score, the cut at 2 x 652 keeps them all > 4096 candidates
#   blocky9600: orb_nfeatures 9600 -> 2 x quota = 4172 candidates on level 0 (4230 with the ties at the cut)
#   mirror_odd_cap256: 500 keypoints leave ANMS, kp_capacity 256
OVERFLOW_CASES = [
    dict(name="tile12", gen="tiled", args=dict(t=12), size=KITTI, nfeatures=3000, anms_num=500, kp_capacity=4096, bits=ST_SEL, may=0),
    dict(name="tile16", gen="tiled", args=dict(t=16), size=KITTI, nfeatures=3000, anms_num=500, kp_capacity=4096, bits=ST_SEL | ST_ANMS, may=0),
    dict(name="blocky3600", gen="blocky", args=dict(seed=0), size=KITTI, nfeatures=3600, anms_num=500, kp_capacity=4096, bits=ST_ANMS, may=0),
    dict(name="binary2", gen="binary", args=dict(block=2), size=KITTI, nfeatures=3000, anms_num=500, kp_capacity=4096, bits=ST_CAND, may=ST_SEL | ST_ANMS),
    dict(name="blocky9600", gen="blocky", args=dict(seed=0), size=KITTI, nfeatures=9600, anms_num=500, kp_capacity=4096, bits=ST_CAND, may=ST_SEL | ST_ANMS),
    dict(name="mirror_odd_cap256", gen="mirror", args=dict(seed=1), size=ODD, nfeatures=1000, anms_num=500, kp_capacity=256, bits=ST_OUT, may=0),
]
OVERFLOW = {c["name"]: c for c in OVERFLOW_CASES}


# the matcher on descriptors of a tiled frame and of the same frame rolled by `shift` columns: oracle = byte-identical descriptor rows beyond the first
# of each kind among the frame's rows (CPU oracle, feature_detection(img, 3000, anms_num)); floor = half of it
MATCHER_TILED = dict(case="tile32", anms_num=1500, shift=7, rows=1500, oracle=763, floor=381)


def duplicate_rows(desc):
    return int(len(desc) - len(np.unique(desc, axis=0)))


# ------------------------------------------------------------------ ANMS helpers
def anms_radii(kps):
    """the suppression radii of visual_odometry.cpp:124-138 in response order (stable), vectorised: (order, radii)"""
    order = np.argsort(-kps["response"], kind="stable")
    k = kps[order]
    x = k["x"].astype(np.float32); y = k["y"].astype(np.float32); r = k["response"].astype(np.float32)
    rad = np.full(len(k), np.finfo(np.float64).max)
    thr = r * np.float32(1.11)
    for i in range(1, len(k)):
        lo = int(np.searchsorted(-r[:i], -thr[i], side="left"))      # r is non-increasing: r[j] > thr for j < lo
        if lo:
            dx = (x[i] - x[:lo]).astype(np.float64); dy = (y[i] - y[:lo]).astype(np.float64)
            rad[i] = np.sqrt((dx * dx + dy * dy).min())
    return order, rad


def anms_tie_nums(kps, want=3):
    """values of num around groups of equal radii: for the largest tie groups (g keypoints sharing the radius ranked a+1 .. a+g from the top)
    num = a (just above the group), a + 1 + g // 2 (inside) and a + g + 1 (just below).  [(num, expected output length)]"""
    _, rad = anms_radii(kps)
    srt = np.sort(rad)[::-1]
    vals, first, cnt = np.unique(-srt, return_index=True, return_counts=True)
    out = []
    for gi in np.argsort(-cnt, kind="stable")[:want]:
        a, g = int(first[gi]), int(cnt[gi])
        if g < 2:
            continue
        for num in (a, a + 1 + g // 2, a + g + 1):
            if 1 <= num <= len(kps):
                out.append((num, int((rad >= srt[num - 1]).sum())))
    return out


def tied_keypoints(n, groups, size=KITTI, seed=0):
    """n user-supplied keypoints on an 8 px lattice (many equal distances) with responses drawn from `groups` distinct values (1: all equal),
    in shuffled order: what the stable (response, input index) order and the radius ties of ANMS have to get right"""
    rng = np.random.default_rng(seed)
    h, w = size
    xs, ys = np.meshgrid(np.arange(32, w - 32, 8), np.arange(32, h - 32, 8))
    pick = rng.permutation(xs.size)[:n]
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = xs.ravel()[pick]; k["y"] = ys.ravel()[pick]; k["size"] = 31; k["angle"] = rng.integers(0, 360, n); k["class_id"] = -1
    k["response"] = (np.float32(1e-3) * np.float32(1.5) ** rng.integers(0, groups, n)).astype(np.float32)
    k["octave"] = rng.integers(0, 3, n)
    return k


def flat_and_symmetric_keypoints():
    """(image, keypoints) pairs for the descriptor on flat and symmetric patches: a constant image (every test compares equal pixels: all bits 0), vertical
    step edges, a checkerboard with keypoints ON the crossings, blob centres; octaves 0..3, angles including 0 / 90 / 180 / 270 exactly"""
    out = []
    h, w = ODD
    for img, pts in ((np.full((h, w), 77, np.uint8), [(60 + 9 * i, 50 + 7 * i) for i in range(20)]),
                     (step_edges(h, w), [(48 + 12 * i, 60 + 5 * i) for i in range(20)]),
                     (checkerboard(h, w, 16), [(48 + 16 * (i % 14), 48 + 16 * (i // 14 * 3)) for i in range(40)]),
                     (blob_lattice(h, w, pitch=30, half=1), [(40 + 30 * (i % 8), 40 + 30 * (i // 8)) for i in range(40)])):
        k = np.zeros(len(pts), KEYPOINT_DTYPE)
        k["x"] = [p[0] for p in pts]; k["y"] = [p[1] for p in pts]; k["size"] = 31; k["response"] = 1; k["class_id"] = -1
        k["octave"] = np.arange(len(pts)) % 4
        k["angle"] = (np.arange(len(pts)) % 8) * 45.0
        out.append((img, k))
    return out
