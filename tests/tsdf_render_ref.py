"""The surface map's ray-cast views in numpy (include/vslam_hip.h "RENDER"): from raw blocks -- what TsdfMap.blocks() returns and load_blocks takes --
to the depth and attribute images of V views, restated exactly.

Every f64 step is ONE numpy float64 operation in the header's order (IEEE, rounded once, no contraction; no `@`, no einsum), every float is cast once
at the end: the device kernels must give these bits in either form.  Nothing is skipped: every ray walks every sample 0 .. K-1 until it ends, every
sample looks its eight corners up.  The pool (slots, probing) is not restated: a field is the blocks it is given.

Next to the images the restatement returns two margins -- the smallest |D| at a known marched sample (the sign decides) and the smallest distance of
a g = Xw / vs - 0.5 of a marched sample from an integer (the floor decides).  The arithmetic is the same on both sides, so they are reported, not
asserted."""
import numpy as np

import tsdf_ref as TR
import voxel_ref as VR

_F = np.float64
MAX_K = 8192


def samples_of(z_min, z_max, hs):
    """K: the smallest non-negative integer with z_min + (double)K * hs >= z_max"""
    z_min, z_max, hs = _F(z_min), _F(z_max), _F(hs)
    K = max(int(np.floor((z_max - z_min) / hs)) - 2, 0)
    while not (z_min + _F(K) * hs >= z_max):
        K += 1
    return K


def _pack(ix, iy, iz):
    return ((ix + VR.HALF) << 36) | ((iy + VR.HALF) << 18) | (iz + VR.HALF)


def tables_of(ids, voxels):
    """map id -> (sorted packed voxel indices, their (W, Sq, Wc, I) rows as int64)"""
    ids = np.asarray(ids, np.int64).reshape(-1, 4)
    vox = np.asarray(voxels).astype(np.int64).reshape(-1, 512, 4)
    l = np.arange(512)
    out = {}
    for m in sorted(set(ids[:, 0].tolist())):
        sel = ids[:, 0] == m
        idx = [(ids[sel, 1 + a, None] * 8 + ((l >> (3 * a)) & 7)[None, :]).ravel() for a in range(3)]
        key = _pack(*idx)
        order = np.argsort(key)
        out[m] = (key[order], vox[sel].reshape(-1, 4)[order])
    return out


def _look(tab, jx, jy, jz, min_w):
    """(good, D, I / Wc) of the voxels (jx, jy, jz) of one map's table; a voxel outside every block is not good"""
    key, rows = tab
    k = _pack(jx, jy, jz)
    pos = np.minimum(np.searchsorted(key, k), len(key) - 1)
    hit = key[pos] == k
    v = np.where(hit[:, None], rows[pos], 0)
    good = hit & (v[:, 0] >= min_w) & (v[:, 0] < TR.MAX_W) & (v[:, 2] >= 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (v[:, 1] - 1024 * v[:, 0]).astype(_F) / v[:, 0].astype(_F)
        inten = v[:, 3].astype(_F) / v[:, 2].astype(_F)
    return good, D, inten


def _lerp(a, b, t):
    return a + t * (b - a)


def sample(tab, Rinv, tinv, x, y, Z, vs, min_w):
    """the sample at depth Z of the rays (x, y): (known, D, (gx, gy, gz), intensity, distance of the nearest g from an integer)"""
    n = len(x)
    Z = np.broadcast_to(np.asarray(Z, _F), (n,))
    with np.errstate(all="ignore"):
        P = (x * Z, y * Z, Z)
        Xw = [Rinv[3 * a] * P[0] + Rinv[3 * a + 1] * P[1] + Rinv[3 * a + 2] * P[2] + tinv[a] for a in range(3)]
        g = [Xw[a] / vs - _F(0.5) for a in range(3)]
        i = [np.floor(g[a]) for a in range(3)]
        f = [g[a] - i[a] for a in range(3)]
        inr = np.ones(n, bool)
        for a in range(3):
            inr &= (i[a] >= -_F(VR.HALF)) & (i[a] + _F(1) < _F(VR.HALF))
    frac = np.full(n, np.inf)
    for a in range(3):
        frac = np.minimum(frac, np.where(inr, np.minimum(f[a], _F(1) - f[a]), np.inf))
    known = inr.copy()
    D = np.zeros(n, _F)
    grad = [np.zeros(n, _F) for _ in range(3)]
    inten = np.zeros(n, _F)
    if tab is None or not inr.any():
        return np.zeros(n, bool), D, grad, inten, frac
    s = np.flatnonzero(inr)
    ii = [i[a][s].astype(np.int64) for a in range(3)]
    Dc, Ic = {}, {}
    ok = np.ones(len(s), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                good, Dv, Iv = _look(tab, ii[0] + dx, ii[1] + dy, ii[2] + dz, min_w)
                ok &= good
                Dc[dx, dy, dz], Ic[dx, dy, dz] = Dv, Iv
    f0, f1, f2 = (f[a][s] for a in range(3))
    with np.errstate(all="ignore"):
        tri = lambda c: _lerp(_lerp(_lerp(c[0, 0, 0], c[1, 0, 0], f0), _lerp(c[0, 1, 0], c[1, 1, 0], f0), f1),
                              _lerp(_lerp(c[0, 0, 1], c[1, 0, 1], f0), _lerp(c[0, 1, 1], c[1, 1, 1], f0), f1), f2)
        Ds, Is = tri(Dc), tri(Ic)
        # the analytic gradient of the interpolant: the differences along the axis, lerped over the other two axes in the order x, y, z
        dX = {(dy, dz): Dc[1, dy, dz] - Dc[0, dy, dz] for dy in (0, 1) for dz in (0, 1)}
        dY = {(dx, dz): Dc[dx, 1, dz] - Dc[dx, 0, dz] for dx in (0, 1) for dz in (0, 1)}
        dZ = {(dx, dy): Dc[dx, dy, 1] - Dc[dx, dy, 0] for dx in (0, 1) for dy in (0, 1)}
        gx = _lerp(_lerp(dX[0, 0], dX[1, 0], f1), _lerp(dX[0, 1], dX[1, 1], f1), f2)
        gy = _lerp(_lerp(dY[0, 0], dY[1, 0], f0), _lerp(dY[0, 1], dY[1, 1], f0), f2)
        gz = _lerp(_lerp(dZ[0, 0], dZ[1, 0], f0), _lerp(dZ[0, 1], dZ[1, 1], f0), f1)
    known[s] = ok
    t = s[ok]
    D[t] = Ds[ok]; inten[t] = Is[ok]
    for a, gv in enumerate((gx, gy, gz)):
        grad[a][t] = gv[ok]
    return known, D, grad, inten, frac


def render(ids, voxels, voxel_size, T, map_id, cam, size, z_min, z_max, march=0.5, min_weight=1):
    """V views of the field: dict(depth (V, h, w) f32, attr (V, h, w, 4) f32 of (nx, ny, nz, intensity), hits, K, margin_D, margin_g)"""
    fx, fy, cx, cy = (_F(v) for v in cam[:4])
    w, h = int(size[0]), int(size[1])
    T = np.asarray(T, _F).reshape(-1, 7)
    map_id = np.asarray(map_id, np.int64).reshape(-1)
    V = len(T)
    vs = _F(np.float32(voxel_size))
    hs = _F(march) * vs
    z_min, z_max = _F(z_min), _F(z_max)
    K = samples_of(z_min, z_max, hs)
    min_w = max(int(min_weight), 1)
    tables = tables_of(ids, voxels)
    depth = np.zeros((V, h * w), np.float32)
    attr = np.zeros((V, h * w, 4), np.float32)
    c, r = np.meshgrid(np.arange(w), np.arange(h))
    x = (c.ravel().astype(_F) - cx) / fx
    y = (r.ravel().astype(_F) - cy) / fy
    margin_D = margin_g = np.inf
    hits = 0
    for v in range(V):
        _, _, Rinv, tinv, finite = TR.frame_of(T[v])
        if not (0 <= map_id[v] <= TR.MAX_MAP and finite):
            continue
        tab = tables.get(int(map_id[v]))
        alive = np.arange(h * w)
        prev = np.zeros(h * w, bool)
        D_prev = np.zeros(h * w, _F)
        for k in range(K):
            if not len(alive):
                break
            Z = z_min + _F(k) * hs
            known, D, _, _, frac = sample(tab, Rinv, tinv, x[alive], y[alive], Z, vs, min_w)
            margin_g = min(margin_g, frac.min())
            if known.any():
                margin_D = min(margin_D, np.abs(D[known]).min())
            pos = known & (D > 0)
            end = known & ~pos
            hit = end & prev[alive]
            if hit.any():
                a = alive[hit]
                with np.errstate(all="ignore"):
                    s = D_prev[a] / (D_prev[a] - D[hit])
                    Zs = (z_min + _F(k - 1) * hs) + s * hs
                depth[v, a] = Zs.astype(np.float32)
                k1, _, g1, i1, _ = sample(tab, Rinv, tinv, x[a], y[a], Zs, vs, min_w)
                _, _, g2, i2, _ = sample(tab, Rinv, tinv, x[a], y[a], Z, vs, min_w)
                g = [np.where(k1, g1[q], g2[q]) for q in range(3)]
                inten = np.where(k1, i1, i2)
                with np.errstate(all="ignore"):
                    norm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
                    flat = ~(np.isfinite(norm) & (norm > 0))
                    for q in range(3):
                        attr[v, a, q] = np.where(flat, _F(0), g[q] / norm).astype(np.float32)
                attr[v, a, 3] = inten.astype(np.float32)
                hits += int(hit.sum())
            prev[alive] = pos
            D_prev[alive] = np.where(pos, D, D_prev[alive])
            alive = alive[~end]
    return dict(depth=depth.reshape(V, h, w), attr=attr.reshape(V, h, w, 4), hits=hits, K=K, margin_D=float(margin_D), margin_g=float(margin_g))


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """T_c_w (qx, qy, qz, qw, tx, ty, tz) of a camera at `eye` whose z axis points at `target` (x right, y down)"""
    eye, target, up = (np.asarray(v, _F) for v in (eye, target, up))
    z = target - eye
    z = z / np.sqrt((z * z).sum())
    x = np.cross(-up, z)
    if (x * x).sum() < 1e-12:
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x = x / np.sqrt((x * x).sum())
    y = np.cross(z, x)
    R = np.stack([x, y, z])                 # rows: the camera axes in the world = R_c_w
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    qw = np.sqrt(max(1.0 + tr, 1e-12)) / 2
    if qw > 1e-3:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * qw), (R[0, 2] - R[2, 0]) / (4 * qw), (R[1, 0] - R[0, 1]) / (4 * qw), qw])
    else:                                    # (a half turn: take the largest diagonal term)
        a = int(np.argmax(np.diag(R)))
        b, c2 = (a + 1) % 3, (a + 2) % 3
        qa = np.sqrt(max(1.0 + R[a, a] - R[b, b] - R[c2, c2], 1e-12)) / 2
        q = np.zeros(4)
        q[a] = qa
        q[b] = (R[b, a] + R[a, b]) / (4 * qa)
        q[c2] = (R[c2, a] + R[a, c2]) / (4 * qa)
        q[3] = (R[c2, b] - R[b, c2]) / (4 * qa)
    q = q / np.sqrt((q * q).sum())
    t = -(R @ eye)
    return np.concatenate([q, t])
