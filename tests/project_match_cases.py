"""Cases for match by projection, shared by the CPU tests of the yardstick (test_project_match_ref.py) and the device parity tests
(test_gpu_project_match.py).

So that no answer can depend on how a device rounds, every case is built away from the bounds of steps 1-3: keypoints sit on a quarter-pixel
lattice, landmarks are back-projected from chosen pixels (lattice + 0.125) at chosen depths, radii are multiples of 0.25 -- so |x_j - u| - r is an odd
multiple of 0.125 up to the ~1e-12 of the back-projection, u and v are 0.125 off the integer borders, and Pz is metres off the gates.
test_project_match_ref.py asserts the margin (>= 1e-6) over all cases.

THE HAND-WORKED CASE (`hand_worked`): 64 x 64 image, K = (100, 100, 32, 32), identity pose, so a point (X, Y, 10) lands on (10 X + 32, 10 Y + 32).
Radius 2, tau 50, ratio 80 %.  Keypoints: k0 (20, 20) descriptor all zero; k1 (22, 20) bits 0-2 of byte 0 set; k2 (40, 40) bytes 0-7 = 0xff; k3 (60, 10)
bytes 8-15 = 0xff.
  L0 -> (21, 20), descriptor: bit 0 of byte 31.  Candidates k0 (|dx| = 1) and k1 (|dx| = 1); k2, k3 are far.  d(k0) = 1, d(k1) = 4.  Best k0 at 1,
        second 4; 1 <= 50; 100 x 1 <= 80 x 4: passes step 4 and claims k0 with key (1, index 0).
  L1 -> (20.5, 20.25), descriptor all zero.  Candidates k0 (0.5, 0.25) and k1 (1.5, 0.25).  d(k0) = 0, d(k1) = 3.  Best k0 at 0, second 3;
        100 x 0 <= 80 x 3: passes and claims k0 with key (0, index 1) -- smaller than L0's.
  L2 -> (40.5, 39.5), descriptor: bytes 0-15 = 0xff.  Candidate k2 only, d = 64 > 50: TOO_FAR.
  Step 5: k0 goes to L1.  Result: status (CONTESTED, MATCHED, TOO_FAR), match (-1, 0, -1), dist (1, 0, 64), n_cand (2, 2, 1)."""
import numpy as np

import project_match_ref as R

K_KITTI = (718.856, 718.856, 607.1928, 185.2157)
FILL = 99   # what the device outputs hold before a call: an item must write its own landmarks and nothing else


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def back_project(T, K4, uv, depth):
    """the world point that T_c_w = T projects onto pixel uv at depth `depth`"""
    P = np.array([(uv[0] - K4[2]) / K4[0] * depth, (uv[1] - K4[3]) / K4[1] * depth, depth])
    return _rot(T[:4]).T @ (P - T[4:])


def random_pose(rng, rot=0.05, trans=0.5):
    q = np.append(rng.normal(0, rot, 3), 1.0)
    return np.append(q / np.linalg.norm(q), rng.normal(0, trans, 3))


IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])


def xor_bits(d, bits):
    d = d.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def flip_bits(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, size=k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def case(name, w, h, items, kps_xy, desc, n, K4=None, src_desc=None, **params):
    """items: list of (img, T, [(xyz, desc_row)])"""
    lm_off = np.cumsum([0] + [len(it[2]) for it in items]).astype(np.int32)
    lms = [lm for it in items for lm in it[2]]
    return dict(name=name, w=w, h=h, K4=K4, lm_off=lm_off, item_img=np.array([it[0] for it in items], np.int32),
                item_T=np.array([it[1] for it in items], np.float64).reshape(-1, 7),
                lm_xyz=np.array([lm[0] for lm in lms], np.float64).reshape(-1, 3), lm_desc_row=np.array([lm[1] for lm in lms], np.int32),
                src_desc=src_desc, kps_xy=np.asarray(kps_xy, np.float32), desc=np.asarray(desc, np.uint8), n=np.asarray(n, np.int32),
                params=dict(dict(radius_px=15.0, tau=50, ratio_pct=80, z_min=0.1, z_max=1e4), **params))


def camera(c):
    return K_KITTI if c["K4"] is None else c["K4"]


def reference(c, margins=None, out=None, **override):
    """the yardstick's answer for a case (parameters overridden by keyword)"""
    src = c["desc"].reshape(-1, 32) if c["src_desc"] is None else c["src_desc"]
    return R.project_match(c["lm_off"], c["item_img"], c["item_T"], c["lm_xyz"], c["lm_desc_row"], src, c["kps_xy"], c["desc"], c["n"], camera(c), c["w"], c["h"],
                           margins=margins, out=out, **dict(c["params"], **override))


def sentinel_out(L):
    return dict(match=np.full(L, FILL, np.int32), dist=np.full(L, FILL, np.int32), n_cand=np.full(L, FILL, np.int32), status=np.full(L, FILL, np.uint8))


# ---------------------------------------------------------------------------------------------------------------- hand-made cases
def hand_worked():
    K4 = (100.0, 100.0, 32.0, 32.0)
    desc = np.zeros((1, 4, 32), np.uint8)
    desc[0, 1, 0] = 0x07; desc[0, 2, :8] = 0xff; desc[0, 3, 8:16] = 0xff
    src = np.zeros((3, 32), np.uint8)
    src[0, 31] = 0x01; src[2, :16] = 0xff
    kps = [[(20, 20), (22, 20), (40, 40), (60, 10)]]
    lms = [(back_project(IDENTITY, K4, uv, 10.0), i) for i, uv in enumerate([(21, 20), (20.5, 20.25), (40.5, 39.5)])]
    return case("hand_worked", 64, 64, [(0, IDENTITY, lms)], kps, desc, [4], K4=K4, src_desc=src, radius_px=2.0)


HAND_WORKED_ANSWER = dict(status=[R.CONTESTED, R.MATCHED, R.TOO_FAR], match=[-1, 0, -1], dist=[1, 0, 64], n_cand=[2, 2, 1])


def every_status():
    """one item that reaches all eight codes; radius 4, tau 50, ratio 80, gate [1, 100]"""
    rng = np.random.default_rng(3)
    K4, T = (100.0, 120.0, 32.0, 30.0), random_pose(rng)
    base = rng.integers(0, 256, (8, 32)).astype(np.uint8)
    kps = [[(10, 10), (30, 30), (50, 50), (50.5, 50.25), (12, 50), (12.5, 50.5), (0, 0), (0, 0)]]
    desc = np.zeros((1, 8, 32), np.uint8)
    desc[0, 0] = base[0]; desc[0, 1] = base[1]; desc[0, 2] = base[2]; desc[0, 3] = flip_bits(rng, base[2], 12); desc[0, 4] = base[4]
    desc[0, 5] = xor_bits(base[4], [200])
    src = np.stack([flip_bits(rng, base[0], 5), flip_bits(rng, base[0], 9), flip_bits(rng, base[1], 70), xor_bits(base[4], range(10)), base[2], base[3]])
    bp = lambda uv, z: back_project(T, K4, uv, z)
    lms = [(bp((10.125, 10.125), 5.0), 0),      # MATCHED: k0 at 5
           (bp((9.625, 10.375), 7.0), 1),       # CONTESTED: k0 at 9, loses to the first
           (bp((30.125, 29.875), 5.0), 2),      # TOO_FAR: k1 at 70
           (bp((12.125, 50.125), 5.0), 3),      # AMBIGUOUS: k4 at 10, k5 at 11: 100 x 10 > 80 x 11
           (bp((40.125, 20.125), 5.0), 4),      # NO_CANDIDATE
           (bp((30.125, 30.125), 150.0), 4),    # BEHIND (past z_max)
           (bp((30.125, 30.125), -5.0), 4),     # BEHIND (behind the camera)
           (bp((-5.125, 30.125), 5.0), 4),      # OUTSIDE
           (np.array([np.nan, 0, 5.0]), 4),     # INVALID (point)
           (bp((50.125, 50.125), 5.0), 77),     # INVALID (row)
           (bp((50.125, 50.125), 5.0), 4)]      # MATCHED: k2 at 0, k3 at 12
    return case("every_status", 64, 64, [(0, T, lms)], kps, desc, [6], K4=K4, src_desc=src, radius_px=4.0, z_min=1.0, z_max=100.0)


# ---------------------------------------------------------------------------------------------------------------- generated cases
def lattice_keypoints(rng, B, cap, n, w, h):
    kps = np.zeros((B, cap, 2), np.float32)
    for b in range(B):
        kps[b, :n[b], 0] = rng.integers(0, 4 * (w - 1) + 1, n[b]) / 4.0
        kps[b, :n[b], 1] = rng.integers(0, 4 * (h - 1) + 1, n[b]) / 4.0
    return kps


def generated(name, seed, w, h, imgs, n_lm, n_kp, cap=None, B=None, K4=None, spread=6, **params):
    """items on images `imgs` with n_lm landmarks each: a landmark aims at a keypoint of its image (lattice + 0.125 + up to `spread` quarter pixels away),
    carries that keypoint's descriptor with 0 .. 70 bits flipped, so that tau, the ratio rule and the claims all decide something; one in sixteen is
    outside the image, one in sixteen outside the depth gate [1, 200], one in sixteen aims at a random pixel"""
    rng = np.random.default_rng(seed)
    B = B if B is not None else max(imgs) + 1
    cap = cap if cap is not None else max(n_kp, 1)
    n = np.full(B, n_kp, np.int32)
    kps = lattice_keypoints(rng, B, cap, n, w, h)
    desc = rng.integers(0, 256, (B, cap, 32)).astype(np.uint8)
    if n_kp >= 8:   # near-duplicates next to each other, for the ratio rule
        for b in range(B):
            for j in range(0, n_kp - 1, 5):
                kps[b, j + 1] = kps[b, j] + np.float32(0.5); desc[b, j + 1] = flip_bits(rng, desc[b, j], int(rng.integers(0, 30)))
        kps[..., 0] = np.clip(kps[..., 0], 0, w - 1); kps[..., 1] = np.clip(kps[..., 1], 0, h - 1)
    Kc = K_KITTI if K4 is None else K4
    items, src = [], []
    for img in imgs:
        T = random_pose(rng)
        lms = []
        for _ in range(n_lm):
            if n_kp:
                j = int(rng.integers(0, n_kp))
                uv = kps[img, j].astype(np.float64) + rng.integers(-spread, spread + 1, 2) * 0.25 + 0.125
                d = flip_bits(rng, desc[img, j], int(rng.choice([0, 2, 10, 30, 49, 50, 51, 70])))
            else:
                uv = np.array([w / 2 + 0.125, h / 2 + 0.125]); d = rng.integers(0, 256, 32).astype(np.uint8)
            depth = float(rng.uniform(2, 50))
            kind = int(rng.integers(0, 16))
            if kind == 0:
                uv = uv + np.array([w + 40.0, 0.0]) * (1 if rng.integers(0, 2) else -1)
            elif kind == 1:
                depth = float(rng.choice([-3.0, 0.5, 250.0]))
            elif kind == 2:   # anywhere in the image: perhaps no keypoint near
                uv = np.array([rng.integers(0, 4 * (w - 2)), rng.integers(0, 4 * (h - 2))]) / 4.0 + 0.125
            lms.append((back_project(T, Kc, uv, depth), len(src)))
            src.append(d)
        items.append((img, T, lms))
    return case(name, w, h, items, kps, desc, n, K4=K4, src_desc=np.array(src, np.uint8).reshape(-1, 32), **dict(dict(z_min=1.0, z_max=200.0), **params))


def cell_borders():
    """keypoints on, and a quarter pixel either side of, the border between grid cells in x and in y; radius 0.5 (inside one cell unless it straddles)"""
    rng = np.random.default_rng(5)
    vals = (31.75, 32.0, 32.25)
    kps = [[(x, y) for y in vals for x in vals]]
    desc = rng.integers(0, 256, (1, 9, 32)).astype(np.uint8)
    K4 = (80.0, 90.0, 31.5, 30.5)
    lms, src = [], []
    for uy in (31.375, 31.875, 32.125, 32.625):
        for ux in (31.375, 31.875, 32.125, 32.625):
            lms.append((back_project(IDENTITY, K4, (ux, uy), 4.0), len(src))); src.append(flip_bits(rng, desc[0, len(src) % 9], 4))
    return case("cell_borders", 64, 64, [(0, IDENTITY, lms)], kps, desc, [9], K4=K4, src_desc=np.array(src), radius_px=0.5, ratio_pct=0)


def image_borders(name="image_borders", w=1241, h=376, K4=None):
    """windows clipped at all four borders and corners of the image, radius 15"""
    rng = np.random.default_rng(6)
    pix = [(0.125, 0.125), (w - 1.125, 0.125), (0.125, h - 1.125), (w - 1.125, h - 1.125), (w / 2 + 0.125, 0.125), (w / 2 + 0.125, h - 1.125),
           (0.125, h // 2 + 0.125), (w - 1.125, h // 2 + 0.125)]
    kps = [[(min(max(round(4 * (u + dx)) / 4, 0), w - 1), min(max(round(4 * (v + dy)) / 4, 0), h - 1)) for (u, v) in pix for dx, dy in ((3, 2), (-3, 5), (14, -14))]]
    desc = rng.integers(0, 256, (1, len(kps[0]), 32)).astype(np.uint8)
    T = random_pose(rng)
    lms = [(back_project(T, K_KITTI if K4 is None else K4, uv, 8.0), 3 * i) for i, uv in enumerate(pix)]
    return case(name, w, h, [(0, T, lms)], kps, desc, [len(kps[0])], K4=K4, ratio_pct=0, tau=255)


def one_keypoint_claimed_by_300():
    """300 landmarks with one descriptor on one pixel: equal distances, the index decides (landmark 0 keeps the keypoint)"""
    rng = np.random.default_rng(7)
    desc = rng.integers(0, 256, (1, 3, 32)).astype(np.uint8)
    kps = [[(100, 100), (400, 200), (800, 300)]]
    src = np.array([flip_bits(rng, desc[0, 1], 7)])
    lms = [(back_project(IDENTITY, K_KITTI, (400.125, 199.875), 3.0 + 0.1 * i), 0) for i in range(300)]
    return case("claimed_by_300", 1241, 376, [(0, IDENTITY, lms)], kps, desc, [3], src_desc=src)


def duplicate_descriptors():
    """every keypoint of the window carries the same descriptor: the smaller keypoint index wins (ratio off; with it on the answer is AMBIGUOUS)"""
    rng = np.random.default_rng(8)
    d = rng.integers(0, 256, 32).astype(np.uint8)
    desc = np.tile(d, (1, 6, 1)); kps = [[(52, 20), (50, 20), (51, 21), (49, 19), (50.5, 20.5), (10, 10)]]
    src = np.array([flip_bits(rng, d, 3), d])
    lms = [(back_project(IDENTITY, (90.0, 90.0, 32.0, 32.0), (50.125, 20.125), 5.0), 0), (back_project(IDENTITY, (90.0, 90.0, 32.0, 32.0), (9.875, 10.125), 5.0), 1)]
    return case("duplicate_descriptors", 64, 64, [(0, IDENTITY, lms)], kps, desc, [6], K4=(90.0, 90.0, 32.0, 32.0), src_desc=src, radius_px=4.0, ratio_pct=0)


def zero_landmarks():
    c = generated("zero_landmarks", 10, 64, 64, [0, 0], 0, 5)
    return c


def same_array():
    """d_src_desc is d_desc itself: a landmark's row is frame x kp_capacity + keypoint"""
    c = generated("same_array", 21, 64, 64, [1, 0], 40, 30, cap=32, B=2, K4=(70.0, 75.0, 32.0, 32.0))
    rng = np.random.default_rng(22)
    c["src_desc"] = None; c["params"]["tau"] = 255
    c["lm_desc_row"] = rng.integers(0, 2 * 32, len(c["lm_desc_row"])).astype(np.int32)
    return c


S = (64, 64)
KS = (60.0, 60.0, 32.0, 32.0)


def all_cases():
    return [hand_worked(), every_status(), zero_landmarks(),
            generated("dn_zero", 11, *S, [0], 5, 0, cap=4, K4=KS),
            generated("one_one", 12, *S, [0], 1, 1, K4=KS, spread=2),
            generated("lm65", 13, *S, [0], 65, 40, K4=KS), generated("lm257", 14, *S, [0], 257, 60, K4=KS),
            cell_borders(), image_borders(), image_borders("image_borders_64", 64, 64, KS),
            generated("radius_half", 15, *S, [0], 80, 50, K4=KS, spread=3, radius_px=0.5), generated("radius_40", 16, 1241, 376, [0], 80, 300, radius_px=40.0),
            one_keypoint_claimed_by_300(), duplicate_descriptors(),
            generated("tau0", 17, *S, [0], 100, 50, K4=KS, tau=0), generated("tau255", 17, *S, [0], 100, 50, K4=KS, tau=255),
            generated("ratio_off", 18, *S, [0], 100, 50, K4=KS, ratio_pct=0), generated("ratio_on", 18, *S, [0], 100, 50, K4=KS, ratio_pct=80),
            generated("two_items_one_image", 19, *S, [0, 0], 70, 40, K4=KS), generated("different_images", 20, *S, [2, 0, 1], 50, 40, K4=KS),
            generated("dn_full", 23, *S, [0, 1], 60, 48, cap=48, K4=KS), same_array(),
            generated("kitti", 24, 1241, 376, [0, 1], 300, 500), generated("fx_ne_fy", 25, 1241, 376, [0], 200, 300, K4=(650.0, 700.0, 600.25, 180.5)),
            generated("random_8x700x900", 26, 1241, 376, [0, 0, 1, 2, 2, 3, 4, 5], 700, 900, cap=912)]


# ---------------------------------------------------------------------------------------------------------------- invalid inputs
def invalid_cases():
    """(case, indices of the landmarks that must come back INVALID): everything else equals the yardstick run on the same arrays"""
    out = []
    base = lambda seed: generated("base", seed, *S, [0, 1, 0], 20, 30, B=2, K4=KS)
    c = base(31); c["name"] = "nan_point"; c["lm_xyz"][[3, 25], [0, 2]] = np.nan, np.inf; out.append((c, [3, 25]))
    c = base(32); c["name"] = "nan_pose"; c["item_T"][1, 5] = np.nan; out.append((c, list(range(20, 40))))
    c = base(33); c["name"] = "row_out_of_range"; c["lm_desc_row"][[0, 59]] = -1, 60; out.append((c, [0, 59]))
    c = base(34); c["name"] = "image_out_of_range"; c["item_img"][[0, 2]] = 2, -1; out.append((c, list(range(0, 20)) + list(range(40, 60))))
    # item 1 = [20, 10) is descending; item 2 = [10, 60) starts below the largest offset before it (20): it writes [20, 60) as INVALID ([10, 20) stays item 0's)
    c = base(35); c["name"] = "descending_lm_off"; c["lm_off"] = np.array([0, 20, 10, 60], np.int32); out.append((c, list(range(20, 60))))
    # an offset past n_landmarks: item 2 = [40, 70) writes [40, 60) as INVALID
    c = base(36); c["name"] = "lm_off_past_the_end"; c["lm_off"] = np.array([0, 20, 40, 70], np.int32); out.append((c, list(range(40, 60))))
    return out
