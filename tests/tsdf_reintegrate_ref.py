"""RE-INTEGRATION of the surface map in numpy (include/vslam_hip.h "RE-INTEGRATION"), on top of the restatement tests/tsdf_ref.py: frames taken out
of the field at the poses they went in with and put in at corrected ones.  The arithmetic is TsdfRef's own -- `_allocate` over the new sides,
`_integrate_frame` into an `add` and a `sub` array -- so the per-sample rule is stated once.  Nothing is culled, as in the parent.

The dict of blocks keeps insertion order, and a call inserts its new blocks after every earlier call's: the position of a block in the dict
is its list position at call granularity (the order INSIDE one call's new blocks is the device's own), which is all that reach needs -- a reach
is the block count after some call's allocation, or a value the rule clamps."""
import numpy as np

import tsdf_ref as TR

_F = np.float64
UNDERFLOW = 8           # status bit 3


class TsdfReintRef(TR.TsdfRef):
    def __init__(self, voxel_size, trunc_voxels, cam):
        super().__init__(voxel_size, trunc_voxels, cam)
        self.n_underflow = 0        # voxels the last reintegrate() left alone
        self.underflowed = []       # ... as (block key, voxel index) of that call

    def reach(self):
        """the number of blocks claimed so far: after integrate() or reintegrate(), the reach of that call's frames"""
        return len(self.blocks)

    def reintegrate(self, disp, gray, T_old, T_new, map_id, reach, z_min, z_max, step=1):
        """one call: disp (B, h, w) float32, gray (B, h, >= w) uint8 or None, T_old / T_new (B, 7), map_id (B,), reach (B,) -> underflowed voxels"""
        disp = np.asarray(disp, np.float32)
        z_min, z_max = _F(z_min), _F(z_max)
        B = len(disp)
        reach = np.broadcast_to(np.asarray(reach, np.int64), (B,))
        old, new = {}, {}
        for b in range(B):
            if not 0 <= int(map_id[b]) <= TR.MAX_MAP:
                continue
            for side, T in ((old, T_old), (new, T_new)):
                R, t, Rinv, tinv, fin = TR.frame_of(T[b])
                if fin:                              # (a side whose pose is not finite is switched off: no count, no status bit)
                    side[b] = (R, t, Rinv, tinv)
        n0 = len(self.blocks)
        for b, fr in new.items():
            self._allocate(disp[b], fr, int(map_id[b]), z_min, z_max, int(step))
        pos = {k: i for i, k in enumerate(self.blocks)}
        self.n_underflow, self.underflowed = 0, []
        for m in sorted({int(map_id[b]) for b in list(old) + list(new)}):
            keys = np.array(sorted(k for k in self.blocks if k[0] == m), np.int64).reshape(-1, 4)
            if not len(keys):
                continue
            p = np.array([pos[tuple(k)] for k in keys.tolist()], np.int64)
            add = np.zeros((len(keys), 512, 4), np.int64)
            sub = np.zeros((len(keys), 512, 4), np.int64)
            for b, fr in new.items():
                if int(map_id[b]) == m:
                    self._integrate_frame(keys, add, disp[b], None if gray is None else gray[b], fr, z_min, z_max)
            for b, fr in old.items():
                if int(map_id[b]) != m:
                    continue
                sel = np.flatnonzero(p < min(int(reach[b]), n0))
                if not len(sel):
                    continue
                part = np.zeros((len(sel), 512, 4), np.int64)
                self._integrate_frame(keys[sel], part, disp[b], None if gray is None else gray[b], fr, z_min, z_max)
                sub[sel] += part
            vox = np.stack([self.blocks[tuple(k)] for k in keys.tolist()])
            under = (vox < sub).any(-1)
            self.n_underflow += int(under.sum())
            self.underflowed += [(tuple(keys[i].tolist()), int(l)) for i, l in np.argwhere(under)]
            vox = np.where(under[..., None], vox, vox + add - sub)
            for k, v in zip(keys.tolist(), vox):
                self.blocks[tuple(k)] = v
        if self.n_underflow:
            self.status |= UNDERFLOW
        return self.n_underflow
