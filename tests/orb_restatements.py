"""numpy restatements of the ORB / ANMS rules, written from the definitions and from the reference's ANMS (visual_odometry.cpp:96-157), independent of
oracle/orb.c: tests/test_oracle_orb.py pins the oracle against them on noise images, tests/test_structured_inputs.py on the tie-dense inputs of
tests/structured_inputs.py."""
import os
import re

import numpy as np

RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_numpy(img, t):
    """FAST-9/16 from the definition: >= 9 contiguous ring pixels all > v+t or all < v-t; score = largest t' that still passes"""
    h, w = img.shape
    I = img.astype(np.int64)
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])  # 16 x (h-6) x (w-6)
    c = I[3:h - 3, 3:w - 3]
    d = c[None] - ring
    ext = np.concatenate([d, d[:8]])
    mins = np.stack([ext[i:i + 9].min(0) for i in range(16)]).max(0)       # best dark arc: all d >= mins
    maxs = np.stack([(-ext[i:i + 9]).min(0) for i in range(16)]).max(0)    # best bright arc
    best = np.maximum(mins, maxs)
    corner = best > t
    return corner, np.maximum(best, t) - 1


def fast_nms_numpy(img, t):
    """FAST-9/16 at threshold t with the 3 x 3 non-maximum suppression of cv::FAST: a corner survives when its score is strictly larger
    than the scores of its eight neighbours (0 where not a corner).  Returns (keep, score), both image-sized."""
    corner, score = fast_numpy(img, t)
    full = np.zeros(img.shape, np.int64); full[3:-3, 3:-3] = np.where(corner, score, 0)
    isc = np.zeros(img.shape, bool); isc[3:-3, 3:-3] = corner
    pad = np.pad(full, 1)
    nb = np.max([pad[1 + dy:pad.shape[0] - 1 + dy, 1 + dx:pad.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)], axis=0)
    return isc & (full > nb), full


def anms_numpy(kps, num):
    """line-by-line numpy/python restatement of visual_odometry.cpp:96-157"""
    if len(kps) < num:
        return kps
    order = np.argsort(-kps["response"], kind="stable")
    k = kps[order]
    rad = np.full(len(k), np.finfo(np.float64).max)
    for i in range(len(k)):
        thr = np.float32(k["response"][i]) * np.float32(1.11)
        j = 0
        while j < i and k["response"][j] > thr:
            dx = np.float32(k["x"][i] - k["x"][j]); dy = np.float32(k["y"][i] - k["y"][j])
            rad[i] = min(rad[i], np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))
            j += 1
    final = np.sort(rad)[::-1][num - 1]
    return k[rad >= final]


def pattern_from_header():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "orb_pattern.h")).read()
    nums = [int(v) for v in re.findall(r"-?\d+", txt.split("= {", 1)[1])]
    return np.array(nums[:1024]).reshape(256, 4)


def retain_best_numpy(response, npoints):
    """KeyPointsFilter::retainBest: indices (input order) of everything >= the npoints-th largest response -- ties at the cut are kept"""
    response = np.asarray(response)
    if npoints < 0 or len(response) <= npoints:
        return np.arange(len(response))
    if npoints == 0:
        return np.arange(0)
    cut = np.sort(response)[::-1][npoints - 1]
    return np.nonzero(response >= cut)[0]


def harris_numpy(img, x0, y0):
    """HarrisResponses of orb.cpp: 3 x 3 Sobel sums over the 7 x 7 block in integers, then float32: (a b - c^2 - 0.04 (a + b)^2) / (4 * 7 * 255)^4"""
    I = img.astype(np.int64)
    a = b = c = 0
    for y in range(y0 - 3, y0 + 4):
        for x in range(x0 - 3, x0 + 4):
            Ix = (I[y, x + 1] - I[y, x - 1]) * 2 + (I[y - 1, x + 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y + 1, x - 1])
            Iy = (I[y + 1, x] - I[y - 1, x]) * 2 + (I[y + 1, x - 1] - I[y - 1, x - 1]) + (I[y + 1, x + 1] - I[y - 1, x + 1])
            a += Ix * Ix; b += Iy * Iy; c += Ix * Iy
    f = np.float32
    scale = f(1.0) / (f(4) * f(7) * f(255)); s4 = scale * scale * scale * scale
    return (f(a) * f(b) - f(c) * f(c) - f(0.04) * (f(a) + f(b)) * (f(a) + f(b))) * s4


UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def ic_moments(img, x, y):
    """(m01, m10) of the intensity centroid over the 31-pixel disc |u| <= UMAX[|v|]"""
    m10 = m01 = 0
    for v in range(-15, 16):
        for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1):
            m10 += u * int(img[y + v, x + u]); m01 += v * int(img[y + v, x + u])
    return m01, m10


def rbrief_numpy(blur, cx, cy, angle_deg, pat=None):
    """the 32 descriptor bytes of computeOrbDescriptors at (cx, cy) of one blurred level: the 256 pattern pairs rotated by the angle, rounded"""
    pat = (pattern_from_header() if pat is None else pat).astype(np.float32)
    f = np.float32
    ang = f(angle_deg) * f(np.pi / 180.0)
    a = f(np.cos(np.float64(ang))); b = f(np.sin(np.float64(ang)))
    bits = []
    for x0, y0, x1, y1 in pat:
        ix0 = int(np.rint(x0 * a - y0 * b)); iy0 = int(np.rint(x0 * b + y0 * a))
        ix1 = int(np.rint(x1 * a - y1 * b)); iy1 = int(np.rint(x1 * b + y1 * a))
        bits.append(int(blur[cy + iy0, cx + ix0]) < int(blur[cy + iy1, cx + ix1]))
    return np.packbits(np.array(bits, np.uint8), bitorder="little")
