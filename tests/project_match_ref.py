"""Plain numpy and Python restatement of match by projection (include/vslam_hip.h "match by projection"): the five steps, with loops, without the grid.
It is the specification the kernel is held to.  Steps 1-3 are f64 in the order the header writes them (Python floats: IEEE doubles, no contraction);
step 4 and 5 are integers, so the device results must equal these bit for bit as long as no compared quantity sits on its bound (the margin
`margins()` reports)."""
import math

import numpy as np

MATCHED, BEHIND, OUTSIDE, NO_CANDIDATE, TOO_FAR, AMBIGUOUS, CONTESTED, INVALID = range(8)
STATUS_NAMES = ("MATCHED", "BEHIND", "OUTSIDE", "NO_CANDIDATE", "TOO_FAR", "AMBIGUOUS", "CONTESTED", "INVALID")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def project(q, X, K4):
    """steps 1 and 2 without the gates: (u, v, Pz); a zero Pz gives non-finite u, v (OUTSIDE, were the gate to let it through)"""
    x, y, z, w = (float(t) for t in q[:4])
    R = ((1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)),
         (2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)),
         (2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)))
    Xw, Yw, Zw = (float(t) for t in X)
    P = [((R[i][0] * Xw + R[i][1] * Yw) + R[i][2] * Zw) + float(q[4 + i]) for i in range(3)]
    fx, fy, cx, cy = (float(t) for t in K4)
    if P[2] == 0.0:
        return math.nan, math.nan, P[2]
    with np.errstate(all="ignore"):
        u = float(np.float64(fx * P[0]) / np.float64(P[2]) + np.float64(cx))
        v = float(np.float64(fy * P[1]) / np.float64(P[2]) + np.float64(cy))
    return u, v, P[2]


def project_match(lm_off, item_img, item_T, lm_xyz, lm_desc_row, src_desc, kps_xy, desc, n, K4, w, h, radius_px=15.0, tau=50, ratio_pct=80,
                  z_min=0.1, z_max=1e4, out=None, margins=None):
    """lm_off (n_items + 1), item_img (n_items), item_T (n_items, 7), lm_xyz (L, 3), lm_desc_row (L), src_desc (rows, 32) uint8, kps_xy (B, cap, 2)
    float32 pixel coordinates, desc (B, cap, 32) uint8, n (B).  Returns dict(match, dist, n_cand int32, status uint8), L each; `out` gives the arrays
    to write into (what no item writes stays as it was).  `margins`, a list, receives |quantity - bound| of every comparison of steps 1-3."""
    lm_off = np.asarray(lm_off, np.int64); item_T = np.asarray(item_T, np.float64).reshape(-1, 7); lm_xyz = np.asarray(lm_xyz, np.float64).reshape(-1, 3)
    src_desc = np.asarray(src_desc, np.uint8).reshape(-1, 32); kps_xy = np.asarray(kps_xy, np.float32); desc = np.asarray(desc, np.uint8)
    B, cap = kps_xy.shape[:2]
    L = len(lm_desc_row)
    if out is None:
        out = dict(match=np.full(L, -1, np.int32), dist=np.full(L, -1, np.int32), n_cand=np.zeros(L, np.int32), status=np.full(L, INVALID, np.uint8))
    r = float(np.float32(radius_px))
    note = (lambda a, b: margins.append(abs(a - b))) if margins is not None else (lambda a, b: None)

    def put(i, status, match=-1, dist=-1, n_cand=0):
        out["status"][i] = status; out["match"][i] = match; out["dist"][i] = dist; out["n_cand"][i] = n_cand

    pm = 0
    for m in range(len(item_img)):
        lo, hi = int(lm_off[m]), int(lm_off[m + 1])
        wlo, whi = max(lo, pm), min(hi, L)
        img = int(item_img[m])
        ok = pm <= lo <= hi <= L and 0 <= img < B and bool(np.isfinite(item_T[m]).all())
        pm = max(pm, lo)
        if not ok:
            for i in range(wlo, whi):
                put(i, INVALID)
            continue
        nk = min(max(int(n[img]), 0), cap)
        passed = {}   # keypoint -> [(d_best, local index, i)]
        for i in range(lo, hi):
            row = int(lm_desc_row[i])
            if not np.isfinite(lm_xyz[i]).all() or not 0 <= row < len(src_desc):
                put(i, INVALID); continue
            u, v, Pz = project(item_T[m], lm_xyz[i], K4)
            note(Pz, z_min); note(Pz, z_max)
            if not z_min <= Pz <= z_max:
                put(i, BEHIND); continue
            for a, b in ((u, 0.0), (u, w - 1.0), (v, 0.0), (v, h - 1.0)):
                note(a, b)
            if not (0 <= u <= w - 1 and 0 <= v <= h - 1):
                put(i, OUTSIDE); continue
            # (every keypoint of the image is looked at: no grid.  float32 -> float64 is exact, the subtraction is one f64 operation)
            dx = np.abs(kps_xy[img, :nk, 0].astype(np.float64) - u); dy = np.abs(kps_xy[img, :nk, 1].astype(np.float64) - v)
            if margins is not None and nk:
                margins.append(float(np.abs(dx - r).min())); margins.append(float(np.abs(dy - r).min()))
            cand = [(hamming(src_desc[row], desc[img, j]), int(j)) for j in np.flatnonzero((dx <= r) & (dy <= r))]
            if not cand:
                put(i, NO_CANDIDATE); continue
            cand.sort()
            d_best, j_best = cand[0]
            if d_best > tau:
                put(i, TOO_FAR, -1, d_best, len(cand))
            elif ratio_pct > 0 and len(cand) > 1 and 100 * d_best > ratio_pct * cand[1][0]:
                put(i, AMBIGUOUS, -1, d_best, len(cand))
            else:
                put(i, CONTESTED, -1, d_best, len(cand))
                passed.setdefault(j_best, []).append((d_best, i - lo, i))
        for j, claims in passed.items():
            i = min(claims)[2]
            out["status"][i] = MATCHED; out["match"][i] = j
    return out
