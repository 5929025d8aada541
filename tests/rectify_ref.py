"""numpy restatement of the rectification stage's arithmetic (include/vslam_hip.h "rectification"), vectorised, written from the published
algorithm of OpenCV's initUndistortRectifyMap(CV_16SC2) + remap(INTER_LINEAR, BORDER_CONSTANT 0) -- PARITY UNPINNED: there is no OpenCV here, so
"equal to this file" is all the tests claim.  Also the rigs the tests run on."""
import numpy as np


def _rot_xyz(rx, ry, rz):
    """R = Rz Ry Rx, angles in degrees"""
    rx, ry, rz = np.deg2rad([rx, ry, rz])
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cam(K, D=(), R=None, P=None):
    D = list(D) + [0.0] * (8 - len(D))
    return dict(K=np.array(K, np.float64), D=np.array(D, np.float64), R=np.eye(3) if R is None else np.array(R, np.float64).reshape(3, 3),
                P=np.array(K if P is None else P, np.float64))


KITTI_K = (718.856, 718.856, 607.1928, 185.2157)
_RAW_K, _RAW_D, _RECT_P = (984.0, 981.0, 690.0, 233.0), (-0.37, 0.20, 1e-3, -6e-4, -0.07, 0.0, 0.0, 0.0), (718.856, 718.856, 607.19, 185.22)
_STRONG_D = (-0.45, 0.12, 5e-4, -3e-4, -0.02, -0.3, 0.05, -0.01)

# name -> src (w, h), dst (w, h), cams (left, right)
RIGS = {
    "identity": dict(src=(1241, 376), dst=(1241, 376), cams=[cam(KITTI_K), cam(KITTI_K)]),
    "kitti_raw_like": dict(src=(1392, 512), dst=(1241, 376),
                           cams=[cam(_RAW_K, _RAW_D, _rot_xyz(0.6, -0.4, 0.3), _RECT_P),
                                 cam((981.5, 979.0, 702.0, 229.5), (-0.36, 0.18, -8e-4, 4e-4, -0.05, 0.0, 0.0, 0.0), _rot_xyz(-0.5, 0.7, -0.2), _RECT_P)]),
    "strong": dict(src=(1241, 376), dst=(1241, 376),
                   cams=[cam(KITTI_K, _STRONG_D, _rot_xyz(0, 0, 5.0), KITTI_K), cam(KITTI_K, _STRONG_D, _rot_xyz(0.3, -0.2, -5.0), KITTI_K)]),
    "small": dict(src=(83, 45), dst=(70, 37),
                  cams=[cam((60.0, 58.0, 41.0, 22.0), (-0.3, 0.1, 2e-3, -1e-3, -0.02), _rot_xyz(1.0, -0.8, 2.0), (52.0, 52.0, 35.5, 18.25)),
                        cam((59.0, 61.0, 40.0, 23.5), (-0.25, 0.05, -1e-3, 2e-3, 0.01), _rot_xyz(-1.2, 0.5, -1.5), (52.0, 52.0, 35.5, 18.25))]),
}


def params_of(pkg, rig):
    """the pkg.RectifyParams of a rig of RIGS (or of a dict of the same shape)"""
    r = RIGS[rig] if isinstance(rig, str) else rig
    return pkg.default_rectify_params(src_w=r["src"][0], src_h=r["src"][1], cams=r["cams"])


def coords32(c, w, h):
    """(32 u, 32 v) in double for every destination pixel of a w x h image: the values the fixed-point map rounds"""
    K, D, R, P = c["K"], c["D"], c["R"], c["P"]
    P3 = np.array([[P[0], 0, P[2]], [0, P[1], P[3]], [0, 0, 1.0]])
    M = np.linalg.inv(P3 @ R)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    with np.errstate(all="ignore"):
        X = M[0, 0] * x + M[0, 1] * y + M[0, 2]; Y = M[1, 0] * x + M[1, 1] * y + M[1, 2]; W = M[2, 0] * x + M[2, 1] * y + M[2, 2]
        xn, yn = X / W, Y / W
        r2 = xn * xn + yn * yn
        k1, k2, p1, p2, k3, k4, k5, k6 = D
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = xn * kr + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
        yd = yn * kr + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
        u = K[0] * xd + K[2]; v = K[1] * yd + K[3]
        return 32 * u, 32 * v


def _fix(c32):
    with np.errstate(all="ignore"):
        i = np.clip(np.rint(np.where(np.isfinite(c32), c32, 0.0)), -2.0 ** 40, 2.0 ** 40).astype(np.int64)   # np.rint: half to even
    return np.clip(i >> 5, -32768, 32767).astype(np.int16), (i & 31).astype(np.uint16)


def build_maps(c, w, h):
    """xy (h, w, 2) int16 and frac (h, w) uint16 = ay * 32 + ax"""
    u32, v32 = coords32(c, w, h)
    sx, ax = _fix(u32); sy, ay = _fix(v32)
    out = ~(np.isfinite(u32) & np.isfinite(v32))
    sx[out] = -32768; sy[out] = -32768; ax[out] = 0; ay[out] = 0
    return np.stack([sx, sy], axis=-1), (ay * 32 + ax).astype(np.uint16)


def near_ties(c, w, h, eps=1e-6):
    """destination pixels where 32 u or 32 v lies within eps of a half-integer: a last-bit difference in the double arithmetic may move the
    fixed-point coordinate by one unit there"""
    u32, v32 = coords32(c, w, h)
    with np.errstate(all="ignore"):
        t = lambda a: np.isfinite(a) & (np.abs(a - np.floor(a) - 0.5) <= eps)
        return t(u32) | t(v32)


def remap(src, xy, frac):
    """src (src_h, src_w) uint8 -> (h, w) uint8; a tap outside the source reads 0, per tap; integers throughout"""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    sx = xy[..., 0].astype(np.int64); sy = xy[..., 1].astype(np.int64)
    ax = (frac & 31).astype(np.int64); ay = ((frac >> 5) & 31).astype(np.int64)

    def S(x, y):
        ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        return np.where(ok, src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64), 0)

    acc = (32 - ax) * (32 - ay) * S(sx, sy) + ax * (32 - ay) * S(sx + 1, sy) + (32 - ax) * ay * S(sx, sy + 1) + ax * ay * S(sx + 1, sy + 1)
    return ((acc + 512) >> 10).astype(np.uint8)


def random_maps(rng, w, h, sw, sh):
    """maps that no lens produces: sx, sy uniform in [-3, src + 2] with independent fractions, a few entries at the int16 limits and at the last
    source column with a fraction -- every border combination of the four taps, and no locality between neighbouring destination pixels"""
    xy = np.stack([rng.integers(-3, sw + 3, (h, w)), rng.integers(-3, sh + 3, (h, w))], axis=-1).astype(np.int16)
    frac = rng.integers(0, 1024, (h, w)).astype(np.uint16)
    xy[0, 0] = (-32768, -32768); xy[0, 1] = (32767, 32767); xy[1, 0] = (-32768, 5); xy[1, 1] = (7, 32767); xy[2, 3] = (32767, -32768)
    xy[3, 5] = (sw - 1, 4); frac[3, 5] = 17 * 32 + 9; xy[3, 6] = (sw - 1, sh - 1); frac[3, 6] = 31 * 32 + 31; xy[4, 2] = (-1, -1); frac[4, 2] = 5 * 32 + 30
    xy[5, 9] = (3, sh - 1); frac[5, 9] = 12 * 32
    for i, sy in enumerate((6, -1, sh - 1, sh + 1)):          # all 4 x 4 combinations of {both taps in, first out, second out, both out} per axis
        for j, sx in enumerate((5, -1, sw - 1, -2)):
            xy[10 + i, 10 + j] = (sx, sy); frac[10 + i, 10 + j] = (3 + 7 * i) * 32 + 5 + 6 * j
    return xy, frac
