"""The surface map stage in numpy (include/vslam_hip.h "surface map"): allocation, integration and extraction of the TSDF, restated exactly.

Every f32 step is a numpy float32 operation, every f64 step ONE numpy float64 operation in the header's order (IEEE, rounded once, no contraction),
the sums are integers: the device kernels must give these bits whatever order frames and blocks arrive in.  Nothing is culled: every block of a
frame's map meets every voxel of it.  The pool (slots, probing, capacity) is not restated: a pool that never fills holds exactly these blocks.

Next to each result the restatement keeps `margin`: the smallest distance of any compared quantity from its decision boundary -- u + 0.5 and
v + 0.5 from an integer, P[2] from vs, z from the gates, sdf from +-tau, sdf * kq from a half-integer -- so that a test can tell an input whose
decisions hang on the last bits of an f64 quotient from one that any correct implementation decides alike."""
import numpy as np

import voxel_ref as VR

MAX_MAP = VR.MAX_MAP
MAX_W = 1 << 20
SURFEL_MAP_DTYPE = np.dtype([("map", "<i4"), ("ix", "<i4"), ("iy", "<i4"), ("iz", "<i4"), ("axis", "<u4"), ("weight", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                             ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("intensity", "<f4")])
_F = np.float64


def rotmat(T):
    """se3::rotmat, operation for operation"""
    x, y, z, w = (_F(v) for v in T[:4])
    tx, ty, tz = _F(2) * x, _F(2) * y, _F(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = _F(1)
    return np.array([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)], _F)


def frame_of(T):
    """(R (9), t (3), Rinv (9), tinv (3), finite) of a pose, as the frame table holds them"""
    T = np.asarray(T, _F)
    with np.errstate(all="ignore"):
        R = rotmat(T)
        Rinv = R[[0, 3, 6, 1, 4, 7, 2, 5, 8]]
        tinv = np.array([-(Rinv[3 * a] * T[4] + Rinv[3 * a + 1] * T[5] + Rinv[3 * a + 2] * T[6]) for a in range(3)], _F)
    return R, T[4:7].copy(), Rinv, tinv, bool(np.isfinite(T).all() and np.isfinite(R).all() and np.isfinite(tinv).all())


def _frac_margin(x):
    """distance of x from the nearest integer"""
    f = x - np.floor(x)
    return np.minimum(f, 1.0 - f)


class TsdfRef:
    """a surface map as a dict of blocks: (map, bx, by, bz) -> (512, 4) int64 of (W, Sq, Wc, I), voxel (ix, iy, iz) at (iz & 7) << 6 | (iy & 7) << 3 | (ix & 7)"""

    def __init__(self, voxel_size, trunc_voxels, cam):
        self.vs32, self.inv = VR.voxel_scale(voxel_size)
        self.vs = _F(self.vs32)
        self.J = int(trunc_voxels)
        self.tau = _F(self.J) * self.vs
        self.kq = _F(1024.0) / self.tau
        self.fx, self.fy, self.cx, self.cy, self.b = (_F(v) for v in cam[:5])
        self.blocks = {}
        self.n_samples = self.n_dropped_range = self.n_frames_skipped = 0
        self.status = 0
        self.margin = np.inf
        self.n_decided = 0      # voxel-frame samples that reached the image lookup

    # ---------------------------------------------------------------------------------------------------------------- allocation
    def _allocate(self, disp, frame, map_id, z_min, z_max, step):
        R, t, Rinv, tinv = frame
        h, w = disp.shape
        rr, cc = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
        d = disp[rr, cc].astype(_F)
        with np.errstate(divide="ignore", invalid="ignore"):
            depth = self.fx * self.b / d
        keep = (depth > z_min) & (depth < z_max)
        fin = np.isfinite(depth)
        if fin.any():
            self.margin = min(self.margin, float(np.minimum(np.abs(depth[fin] - z_min), np.abs(depth[fin] - z_max)).min()))
        depth, cc, rr = depth[keep], cc[keep], rr[keep]
        x = (cc.astype(np.float32).astype(_F) - self.cx) / self.fx
        y = (rr.astype(np.float32).astype(_F) - self.cy) / self.fy
        new = set()
        for j in range(-self.J, self.J + 1):
            Z = depth + _F(j) * self.vs
            ok = ~(Z <= 0)
            X = x * Z; Y = y * Z
            idx = []
            inr = ok.copy()
            for a in range(3):
                p = (Rinv[3 * a] * X + Rinv[3 * a + 1] * Y + Rinv[3 * a + 2] * Z + tinv[a]).astype(np.float32)
                oka, i, _ = VR.axis_key(p, self.inv)
                inr &= oka
                idx.append(i)
            self.n_dropped_range += int((ok & ~inr).sum())
            self.n_samples += int(inr.sum())
            bl = np.stack([i[inr] >> 3 for i in idx], 1)
            new.update(map(tuple, np.unique(bl, axis=0).tolist()))
        for bl in new:
            self.blocks.setdefault((int(map_id),) + bl, np.zeros((512, 4), np.int64))

    # ---------------------------------------------------------------------------------------------------------------- integration
    def _integrate_frame(self, keys, vox, disp, gray, frame, z_min, z_max):
        """one frame into the blocks `keys` (n, 4) of its map; vox (n, 512, 4) is updated in place"""
        R, t, _, _ = frame
        h, w = disp.shape
        vs, tau, kq = self.vs, self.tau, self.kq
        l = np.arange(512)
        i = [keys[:, 1 + a, None] * 8 + ((l >> (3 * a)) & 7)[None, :] for a in range(3)]       # (n, 512) voxel indices per axis
        X = [(ia.astype(_F) + _F(0.5)) * vs for ia in i]
        P = [R[3 * a] * X[0] + R[3 * a + 1] * X[1] + R[3 * a + 2] * X[2] + t[a] for a in range(3)]
        self.margin = min(self.margin, float(np.abs(P[2] - vs).min()))
        m = P[2] > vs
        sel = np.nonzero(m)
        P0, P1, P2 = P[0][sel], P[1][sel], P[2][sel]
        u = self.fx * (P0 / P2) + self.cx
        v = self.fy * (P1 / P2) + self.cy
        uh, vh = u + _F(0.5), v + _F(0.5)
        cf, rf = np.floor(uh), np.floor(vh)
        # (a voxel far outside the image decides nothing on the last bits: only those within a pixel of the image count towards the margin)
        near = (uh > -1) & (uh < w + 1) & (vh > -1) & (vh < h + 1)
        if near.any():
            self.margin = min(self.margin, float(_frac_margin(uh[near]).min()), float(_frac_margin(vh[near]).min()))
        ins = (cf >= 0) & (cf < w) & (rf >= 0) & (rf < h)
        sel = tuple(s[ins] for s in sel)
        c, r, P2 = cf[ins].astype(np.int64), rf[ins].astype(np.int64), P2[ins]
        self.n_decided += len(c)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = self.fx * self.b / disp[r, c].astype(_F)
        fin = np.isfinite(z)
        if fin.any():
            self.margin = min(self.margin, float(np.minimum(np.abs(z[fin] - z_min), np.abs(z[fin] - z_max)).min()))
        g = (z > z_min) & (z < z_max)
        sel = tuple(s[g] for s in sel)
        c, r, z, P2 = c[g], r[g], z[g], P2[g]
        sdf = z - P2
        if len(sdf):
            self.margin = min(self.margin, float(np.minimum(np.abs(sdf - tau), np.abs(sdf + tau)).min()))
        front = ~(sdf < -tau)
        sel = tuple(s[front] for s in sel)
        c, r, sdf = c[front], r[front], sdf[front]
        s = np.minimum(sdf, tau) * kq
        if len(s):
            self.margin = min(self.margin, float(np.abs(_frac_margin(s) - 0.5).min()))
        q = np.rint(s).astype(np.int64)
        assert len(q) == 0 or (q.min() >= -1024 and q.max() <= 1024)
        close = sdf <= tau
        inten = gray[r, c].astype(np.int64) if gray is not None else np.zeros(len(c), np.int64)
        # (each voxel appears at most once per frame: plain fancy-index adds are exact)
        vox[sel[0], sel[1], 0] += 1
        vox[sel[0], sel[1], 1] += q + 1024
        vox[sel[0], sel[1], 2] += close
        vox[sel[0], sel[1], 3] += np.where(close, inten, 0)

    def integrate(self, disp, gray, T, map_id, z_min, z_max, step=1):
        """one call: disp (B, h, w) float32, gray (B, h, >= w) uint8 or None, T (B, 7), map_id (B,)"""
        disp = np.asarray(disp, np.float32)
        z_min, z_max = _F(z_min), _F(z_max)
        frames = {}
        for b in range(len(disp)):
            if not 0 <= int(map_id[b]) <= MAX_MAP:
                continue
            R, t, Rinv, tinv, fin = frame_of(T[b])
            if not fin:
                self.n_frames_skipped += 1
                self.status |= 4
                continue
            frames[b] = (R, t, Rinv, tinv)
        for b, fr in frames.items():
            self._allocate(disp[b], fr, int(map_id[b]), z_min, z_max, int(step))
        for m in sorted({int(map_id[b]) for b in frames}):
            keys = np.array(sorted(k for k in self.blocks if k[0] == m), np.int64).reshape(-1, 4)
            if not len(keys):
                continue
            vox = np.stack([self.blocks[tuple(k)] for k in keys.tolist()])
            for b, fr in frames.items():
                if int(map_id[b]) == m:
                    self._integrate_frame(keys, vox, disp[b], None if gray is None else gray[b], fr, z_min, z_max)
            for k, v in zip(keys.tolist(), vox):
                self.blocks[tuple(k)] = v

    # ---------------------------------------------------------------------------------------------------------------- read-out
    def dump(self, map_id=-1):
        """(ids (n, 4) int32, voxels (n, 512, 4) uint32) sorted by (map, bx, by, bz): TsdfMap.blocks()"""
        keys = sorted(k for k in self.blocks if map_id < 0 or k[0] == map_id)
        ids = np.array(keys, np.int32).reshape(-1, 4)
        vox = np.stack([self.blocks[k] for k in keys]).astype(np.uint32) if keys else np.zeros((0, 512, 4), np.uint32)
        return ids, vox

    def voxel(self, map_id, ix, iy, iz):
        """(W, Sq, Wc, I) of one voxel, zeros if no block holds it"""
        blk = self.blocks.get((map_id, ix >> 3, iy >> 3, iz >> 3))
        return np.zeros(4, np.int64) if blk is None else blk[(iz & 7) << 6 | (iy & 7) << 3 | (ix & 7)]

    def extract(self, map_id=-1, min_weight=1):
        """the crossing edges of map map_id (-1: all) as SURFEL_MAP_DTYPE, sorted by (map, ix, iy, iz, axis)"""
        ids, vox = self.dump(map_id)
        out = []
        for m in sorted(set(ids[:, 0].tolist())):
            out.append(self._extract_map(m, ids[ids[:, 0] == m], vox[ids[:, 0] == m].astype(np.int64), max(int(min_weight), 1)))
        out = np.concatenate(out) if out else np.zeros(0, SURFEL_MAP_DTYPE)
        return out[np.lexsort((out["axis"], out["iz"], out["iy"], out["ix"], out["map"]))]

    def _extract_map(self, m, ids, vox, min_w):
        # every voxel of the map in one sorted table: packed index -> row
        l = np.arange(512)
        idx = [(ids[:, 1 + a, None].astype(np.int64) * 8 + ((l >> (3 * a)) & 7)[None, :]).ravel() for a in range(3)]
        pack = lambda ix, iy, iz: ((ix + VR.HALF) << 36) | ((iy + VR.HALF) << 18) | (iz + VR.HALF)
        key = pack(*idx)
        order = np.argsort(key)
        key = key[order]
        tab = vox.reshape(-1, 4)[order]
        ix, iy, iz = (a[order] for a in idx)
        if (tab[:, 0] >= MAX_W).any():
            self.status |= 2

        def look(jx, jy, jz):
            """(good, num, D, rows) of the voxels (jx, jy, jz); a voxel outside the range or outside every block is not good"""
            inr = (np.abs(jx + 0.5) < VR.HALF) & (np.abs(jy + 0.5) < VR.HALF) & (np.abs(jz + 0.5) < VR.HALF)
            k = pack(jx, jy, jz)
            pos = np.minimum(np.searchsorted(key, k), len(key) - 1)
            hit = inr & (key[pos] == k)
            v = np.where(hit[:, None], tab[pos], 0)
            good = hit & (v[:, 0] >= min_w) & (v[:, 0] < MAX_W) & (v[:, 2] >= 1)
            num = v[:, 1] - 1024 * v[:, 0]
            with np.errstate(divide="ignore", invalid="ignore"):
                D = num.astype(_F) / v[:, 0].astype(_F)
            return good, num, D, v

        good_a, num_a, D_a, v_a = look(ix, iy, iz)
        out = []
        vs = self.vs
        for e in range(3):
            de = [int(e == a) for a in range(3)]
            good_b, num_b, D_b, v_b = look(ix + de[0], iy + de[1], iz + de[2])
            cross = good_a & good_b & ((num_a > 0) != (num_b > 0))
            s = np.nonzero(cross)[0]
            a_idx = [ix[s], iy[s], iz[s]]
            Da, Db = D_a[s], D_b[s]
            t = Da / (Da - Db)
            g = [None] * 3
            g[e] = Db - Da
            for k in (1, 2):
                f = (e + k) % 3
                df = [int(f == a) for a in range(3)]
                tot = np.zeros(len(s), _F)
                n = np.zeros(len(s), np.int64)
                for c in (0, 1):
                    cx, cy, cz = (a_idx[a] + c * de[a] for a in range(3))
                    gp, _, Dp, _ = look(cx + df[0], cy + df[1], cz + df[2])
                    gm, _, Dm, _ = look(cx - df[0], cy - df[1], cz - df[2])
                    both = gp & gm
                    with np.errstate(invalid="ignore"):
                        term = (Dp - Dm) / _F(2.0)
                    tot = np.where(both, tot + np.where(both, term, 0), tot)
                    n += both
                with np.errstate(divide="ignore", invalid="ignore"):
                    g[f] = np.where(n > 0, tot / n.astype(_F), _F(0))
            norm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
            r = np.zeros(len(s), SURFEL_MAP_DTYPE)
            r["map"] = m
            r["ix"], r["iy"], r["iz"] = a_idx
            r["axis"] = e
            r["weight"] = np.minimum(v_a[s, 0], v_b[s, 0])
            for a, name in enumerate("xyz"):
                base = a_idx[a].astype(_F) + _F(0.5)
                r[name] = ((base + t if a == e else base) * vs).astype(np.float32)
                r["n" + name] = (g[a] / norm).astype(np.float32)
            r["intensity"] = ((v_a[s, 3].astype(_F) + v_b[s, 3].astype(_F)) / (v_a[s, 2].astype(_F) + v_b[s, 2].astype(_F))).astype(np.float32)
            out.append(r)
        return np.concatenate(out)
