"""The chained BA of throughput mode (vslam_ba_chain_dev) restated in numpy, independently of the library: which windows run at which step, what a
step's staging batch looks like, what enters a window (carried poses and is_inlier flags), what goes back, and what an inactive window passes through.
The optimiser itself is a callback, so the same composer serves the CPU tests (the oracle's schedule) and the GPU tests (vslam_ba_batch_dev).

Contract (include/vslam_hip.h): step j runs window first[s] + j of every sequence s with more than j frames, in ascending sequence order.
Window w, n_k = n_kf_w[w] keyframes, frames kf_frame[w][:n_k]:
  entry   slot k of frame g != w takes the pose the chain holds for g (if any window left one), the slot of w keeps the builder's pose;
          lm_inlier[l] = the chain's flag of lm_id[l] (1 until written);
  active  (n_k >= min_kf, n_k >= 1): runs from the entry state; poses of the first n_k slots and the flags go to the caller's arrays and the state;
  passive (0 < n_k < min_kf): the entry poses / flags are written to the caller's arrays, the window's own pose enters the state;
  empty   (n_k = 0): left as built.
A window that does not run contributes an EMPTY staging window: offsets do not advance, n_kf 0, the builder's poses."""
import numpy as np


def sliding_sets(first, n_kf):
    """kf_frame (W, n_kf) of the sliding windows, restarted at every sequence's first frame; -1 in unused slots"""
    W = int(first[-1])
    kf = np.full((W, n_kf), -1, np.int32)
    for lo, hi in zip(first[:-1], first[1:]):
        for w in range(lo, hi):
            fr = np.arange(max(lo, w - n_kf + 1), w + 1)
            kf[w, :len(fr)] = fr
    return kf


def compose(batch, lm_id, kf_frame, first, min_kf, run):
    """batch: dict(n_kf, lm_off (W + 1), e_off (W + 1), nkf (W), T (W, n_kf, 7), xyz (L, 3), rel (L), inl (L), kf (E), lm (E), uv (E, 2)) -- a builder's
    output for the whole batch; lm_id (L); kf_frame (W, n_kf) or None (sliding); first (n_seg + 1); run(staging) -> dict(T (n, n_kf, 7), inl (l),
    status (n)) for a staging dict of the same keys plus n_windows.  Returns dict(T, inl, ran, status, steps) -- steps: every staging batch, for tests."""
    n_kf = int(batch["n_kf"])
    first = np.asarray(first, np.int64)
    W = int(first[-1])
    lm_off, e_off, nkf = (np.asarray(batch[k], np.int64) for k in ("lm_off", "e_off", "nkf"))
    if kf_frame is None:
        kf_frame = sliding_sets(first, n_kf)
    T = np.array(batch["T"], np.float64).reshape(W, n_kf, 7).copy()
    inl = np.array(batch["inl"], np.uint8).copy()
    ran = np.zeros(W, np.int32); status = np.zeros(W, np.int32)
    pose, flag = {}, {}
    lens = np.diff(first)
    steps = []
    for j in range(int(lens.max())):
        slots = [int(first[s]) + j for s in range(len(lens)) if lens[s] > j]
        st = dict(n_windows=len(slots), n_kf=n_kf, lm_off=[0], e_off=[0], nkf=[], T=[], xyz=[], rel=[], inl=[], kf=[], lm=[], uv=[], windows=slots)
        for w in slots:
            nk = int(nkf[w]); l0, l1, e0, e1 = lm_off[w], lm_off[w + 1], e_off[w], e_off[w + 1]
            frames = [int(g) for g in kf_frame[w][:nk]]
            built = T[w].copy()
            entry_T = built.copy()
            for k, g in enumerate(frames):
                if g != w and g in pose:
                    entry_T[k] = pose[g]
            entry_inl = np.array([flag.get(int(i), 1) for i in lm_id[l0:l1]], np.uint8)
            active = nk >= 1 and nk >= min_kf
            if active:
                st["T"].append(entry_T); st["nkf"].append(nk)
                st["xyz"].append(batch["xyz"][l0:l1]); st["rel"].append(batch["rel"][l0:l1]); st["inl"].append(entry_inl)
                st["kf"].append(batch["kf"][e0:e1]); st["lm"].append(batch["lm"][e0:e1]); st["uv"].append(batch["uv"][e0:e1])
                st["lm_off"].append(st["lm_off"][-1] + int(l1 - l0)); st["e_off"].append(st["e_off"][-1] + int(e1 - e0))
                continue
            st["T"].append(built); st["nkf"].append(0)
            st["lm_off"].append(st["lm_off"][-1]); st["e_off"].append(st["e_off"][-1])
            if nk > 0:
                T[w][:nk] = entry_T[:nk]; inl[l0:l1] = entry_inl
                if w in frames:
                    pose[w] = built[frames.index(w)].copy()
        cat = lambda xs, shape, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt)
        staging = dict(n_windows=len(slots), n_kf=n_kf, windows=slots, lm_off=np.array(st["lm_off"], np.int32), e_off=np.array(st["e_off"], np.int32),
                       nkf=np.array(st["nkf"], np.int32), T=np.stack(st["T"]), xyz=cat(st["xyz"], (0, 3), np.float32), rel=cat(st["rel"], (0,), np.uint8),
                       inl=cat(st["inl"], (0,), np.uint8), kf=cat(st["kf"], (0,), np.int32), lm=cat(st["lm"], (0,), np.int32),
                       uv=cat(st["uv"], (0, 2), np.float32))
        steps.append(staging)
        res = run(staging)
        for i, w in enumerate(slots):
            nk = int(staging["nkf"][i])
            if nk == 0:
                continue
            T[w][:nk] = res["T"][i][:nk]
            for k, g in enumerate(int(g) for g in kf_frame[w][:nk]):
                pose[g] = np.array(res["T"][i][k], np.float64)
            got = np.asarray(res["inl"][staging["lm_off"][i]:staging["lm_off"][i + 1]], np.uint8)
            l0, l1 = lm_off[w], lm_off[w + 1]
            inl[l0:l1] = got
            for i_, v in zip(lm_id[l0:l1], got):
                flag[int(i_)] = int(v)
            ran[w] = 1; status[w] = int(res["status"][i])
    return dict(T=T, inl=inl, ran=ran, status=status, steps=steps)


def oracle_schedule(oracle, T, xyz, rel, kf, lm, uv, inl=None, margins=None):
    """the reference's per-keyframe schedule (run_vslam.cpp:58-71) on one window with the oracle's optimisers -- the composite of
    tests/test_gpu_windows_kf._oracle_schedule, taking the incoming is_inlier flags (None: all 1).  margins (a list): receives, per classification,
    min |chi2 - threshold| / threshold over the classified edges."""
    inl = np.ones(len(xyz), np.uint8) if inl is None else np.array(inl, np.uint8).copy()
    rel = np.asarray(rel).astype(bool)

    def classify(chi2, lms, inl):
        th, inl, _, _ = oracle.chi2_classify(chi2, lms, inl)
        if margins is not None and len(chi2):
            margins.append(float(np.min(np.abs(chi2 - th)) / th))
        return inl
    for iters, upd in ((5, False), (5, False), (10, True)):
        act = (inl.astype(bool) & rel)[lm]
        T2, _, chi2, _ = oracle.local_ba(T, xyz, kf[act], lm[act], uv[act], iters=iters)
        inl = classify(chi2, lm[act], inl)
        if upd:
            T = T2
    act = inl.astype(bool)[lm]
    T2, chi2, _ = oracle.pose_only_window(T, xyz, kf[act], lm[act], uv[act], iters=10)
    inl = classify(chi2, lm[act], inl)
    return T2, inl


def oracle_run(oracle, margins=None):
    """a compose() callback: every non-empty staging window through oracle_schedule"""
    def run(st):
        T = st["T"].copy(); inl = st["inl"].copy()
        for i in range(st["n_windows"]):
            nk = int(st["nkf"][i])
            if nk == 0:
                continue
            l0, l1, e0, e1 = st["lm_off"][i], st["lm_off"][i + 1], st["e_off"][i], st["e_off"][i + 1]
            T2, got = oracle_schedule(oracle, st["T"][i][:nk].copy(), st["xyz"][l0:l1], st["rel"][l0:l1], st["kf"][e0:e1], st["lm"][e0:e1], st["uv"][e0:e1],
                                      inl=st["inl"][l0:l1], margins=margins)
            T[i][:nk] = T2; inl[l0:l1] = got
        return dict(T=T, inl=inl, status=np.zeros(st["n_windows"], np.int32))
    return run
