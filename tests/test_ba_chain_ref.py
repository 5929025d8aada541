"""CPU: the step composer of the chained BA (tests/ba_chain_ref.py) with the oracle's schedule as its optimiser, on small hand-built sliding
windows (3 keyframes, 20 landmarks, n_kf = 3): what is carried from window to window, what an inactive window passes through, and that sequences
laid back to back do not see each other.  The GPU entry (vslam_ba_chain_dev) is held to this composer bit for bit in tests/test_gpu_ba_chain.py."""
import numpy as np

import ba_chain_ref as CR

N_KF, N_LM = 3, 20
K = (718.856, 718.856, 607.1928, 185.2157)


def _sequence(O, seed, F=5, id0=0, outlier=None):
    """F frames moving forward and sideways past N_LM points, every point seen in every frame; window w = frames [max(0, w - 2), w] at the pose-stage
    poses G (truth plus a small error, the same in every window that holds the frame).  outlier = (frame, landmark): that observation is off by 75 px."""
    rng = np.random.default_rng(seed)
    pts = np.c_[rng.uniform(-8, 8, N_LM), rng.uniform(-3, 3, N_LM), rng.uniform(12, 30, N_LM)]
    true = [O.se3_exp(np.array([-0.3 * f, 0.02 * f, -0.5 * f, 0.0, 0.01 * f, 0.0])) for f in range(F)]
    G = [true[0]] + [O.se3_mul(O.se3_exp(np.r_[rng.normal(0, 0.03, 3), rng.normal(0, 0.003, 3)]), true[f]) for f in range(1, F)]
    obs = np.zeros((F, N_LM, 2), np.float32)
    for f in range(F):
        for l in range(N_LM):
            p = O.se3_act(true[f], pts[l])
            obs[f, l] = (K[0] * p[0] / p[2] + K[2] + rng.normal(0, 0.3), K[1] * p[1] / p[2] + K[3] + rng.normal(0, 0.3))
    if outlier is not None:
        obs[outlier[0], outlier[1]] += (60.0, -45.0)
    xyz = (pts + rng.normal(0, 0.004, pts.shape)).astype(np.float32)   # (well under a pixel at these depths)
    rel = np.ones(N_LM, np.uint8); rel[[3, 11]] = 0
    b = dict(n_kf=N_KF, lm_off=[0], e_off=[0], nkf=[], T=[], xyz=[], rel=[], inl=[], kf=[], lm=[], uv=[])
    ids = []
    for w in range(F):
        frames = list(range(max(0, w - N_KF + 1), w + 1))
        Tw = np.zeros((N_KF, 7)); Tw[:, 3] = 1
        Tw[:len(frames)] = [G[f] for f in frames]
        b["T"].append(Tw); b["nkf"].append(len(frames))
        b["xyz"].append(xyz); b["rel"].append(rel); b["inl"].append(np.ones(N_LM, np.uint8)); ids.append(id0 + 5 * np.arange(N_LM))
        for l in range(N_LM):   # landmark-major, chronological inside a landmark
            for k, f in enumerate(frames):
                b["kf"].append(k); b["lm"].append(l); b["uv"].append(obs[f, l])
        b["lm_off"].append(b["lm_off"][-1] + N_LM); b["e_off"].append(len(b["kf"]))
    out = dict(n_kf=N_KF, lm_off=np.array(b["lm_off"], np.int32), e_off=np.array(b["e_off"], np.int32), nkf=np.array(b["nkf"], np.int32), T=np.stack(b["T"]),
               xyz=np.concatenate(b["xyz"]), rel=np.concatenate(b["rel"]), inl=np.concatenate(b["inl"]), kf=np.array(b["kf"], np.int32),
               lm=np.array(b["lm"], np.int32), uv=np.array(b["uv"], np.float32))
    return out, np.concatenate(ids).astype(np.int32)


def _independent(O, b):
    """every window on its own from the builder's state: what vslam_ba_batch_dev computes"""
    F = len(b["nkf"])
    return CR.compose(b, np.arange(len(b["xyz"]), dtype=np.int32), CR.sliding_sets(np.array([0, F]), N_KF), np.arange(F + 1), 1, CR.oracle_run(O))   # (every window a sequence of its own, no id shared)


def test_schedule_composite_is_the_existing_one(oracle):
    """oracle_schedule with no incoming flags is tests/test_gpu_windows_kf._oracle_schedule"""
    import test_gpu_windows_kf as W
    b, _ = _sequence(oracle, 1)
    w = 3
    l0, l1, e0, e1 = b["lm_off"][w], b["lm_off"][w + 1], b["e_off"][w], b["e_off"][w + 1]
    args = (b["T"][w].copy(), b["xyz"][l0:l1], b["rel"][l0:l1].astype(bool), b["kf"][e0:e1], b["lm"][e0:e1], b["uv"][e0:e1])
    T1, i1 = W._oracle_schedule(oracle, *args)
    T2, i2 = CR.oracle_schedule(oracle, *args)
    assert np.array_equal(T1, T2) and np.array_equal(i1, i2)


def test_min_kf_above_every_window_passes_through(oracle):
    b, ids = _sequence(oracle, 2)
    calls = []
    inner = CR.oracle_run(oracle)
    def run(st):
        calls.append(int(st["nkf"].sum()))
        return inner(st)
    r = CR.compose(b, ids, None, [0, 5], N_KF + 1, run)
    assert np.array_equal(r["T"], b["T"]) and np.array_equal(r["inl"], b["inl"])
    assert (r["ran"] == 0).all() and (r["status"] == 0).all() and calls == [0] * 5
    for st in r["steps"]:   # an inactive sequence contributes an empty window holding the builder's poses
        assert st["n_windows"] == 1 and st["lm_off"].tolist() == [0, 0] and st["e_off"].tolist() == [0, 0] and st["nkf"].tolist() == [0]
        assert np.array_equal(st["T"][0], b["T"][st["windows"][0]])


def test_outlier_flag_is_carried(oracle):
    """landmark 7's observation in frame 2 is a gross outlier: window 2 (where it is the landmark's last edge) flags it, window 3 runs without the
    landmark, and that changes window 3's result"""
    j, L = 2, 7
    b, ids = _sequence(oracle, 3, outlier=(j, L))
    r = CR.compose(b, ids, None, [0, 5], 1, CR.oracle_run(oracle))
    assert (r["ran"] == 1).all()
    assert r["inl"][b["lm_off"][j] + L] == 0
    nxt = r["steps"][j + 1]
    assert nxt["windows"] == [j + 1] and nxt["inl"][L] == 0 and nxt["inl"].sum() >= N_LM - 3
    assert r["inl"][b["lm_off"][j + 1] + L] == 0   # never in a graph again, so never reclassified
    # the same entry poses with every flag 1: another result
    T_all, inl_all = CR.oracle_schedule(oracle, nxt["T"][0].copy(), nxt["xyz"], nxt["rel"], nxt["kf"], nxt["lm"], nxt["uv"])
    assert not np.array_equal(T_all, r["T"][j + 1]) and np.abs(T_all - r["T"][j + 1]).max() > 1e-9
    # and the independent windows differ from the chained ones from window 1 on (poses), window 0 being the same
    ind = _independent(oracle, b)
    assert np.array_equal(ind["T"][0], r["T"][0]) and not np.array_equal(ind["T"][j + 1], r["T"][j + 1])


def test_shared_keyframe_enters_at_the_previous_output(oracle):
    b, ids = _sequence(oracle, 4)
    r = CR.compose(b, ids, None, [0, 5], 1, CR.oracle_run(oracle))
    kf = CR.sliding_sets(np.array([0, 5]), N_KF)
    out_prev = None
    for j, st in enumerate(r["steps"]):
        nk = int(st["nkf"][0])
        frames = kf[j][:nk].tolist()
        assert frames[-1] == j and np.array_equal(st["T"][0][nk - 1], b["T"][j][nk - 1])   # the new keyframe: the builder's pose
        if out_prev is not None:
            for k, g in enumerate(frames[:-1]):
                assert np.array_equal(st["T"][0][k], out_prev[g]), (j, g)   # bit for bit
                assert not np.array_equal(st["T"][0][k], b["T"][j][k]) or g == 0
        res_T = r["T"][j] if j == len(r["steps"]) - 1 else None
        # what window j wrote: recompute from its staging batch
        T2, _ = CR.oracle_schedule(oracle, st["T"][0][:nk].copy(), st["xyz"], st["rel"], st["kf"], st["lm"], st["uv"], inl=st["inl"])
        out_prev = {g: T2[k] for k, g in enumerate(frames)}
        if res_T is not None:
            assert np.array_equal(res_T[:nk], T2)
    # min_kf = 3: windows 0 and 1 pass through, window 2 is the first to run and starts from the builder's poses
    r3 = CR.compose(b, ids, None, [0, 5], 3, CR.oracle_run(oracle))
    assert r3["ran"].tolist() == [0, 0, 1, 1, 1]
    assert np.array_equal(r3["steps"][2]["T"][0], b["T"][2]) and np.array_equal(r3["T"][1], b["T"][1])


def test_sequences_back_to_back(oracle):
    """two sequences in one batch give what each gives alone; the second one's ids and frames are offset, and an id the two share by accident would
    couple them -- the composer keys flags by id, so the test keeps them disjoint as the builder does (frame x kp_capacity + keypoint)"""
    a, ida = _sequence(oracle, 5, F=5, outlier=(1, 4))
    c, idc = _sequence(oracle, 6, F=4, id0=1000, outlier=(2, 9))
    both = dict(n_kf=N_KF, lm_off=np.concatenate([a["lm_off"], a["lm_off"][-1] + c["lm_off"][1:]]), e_off=np.concatenate([a["e_off"], a["e_off"][-1] + c["e_off"][1:]]),
                nkf=np.concatenate([a["nkf"], c["nkf"]]), T=np.concatenate([a["T"], c["T"]]))
    for k in ("xyz", "rel", "inl", "kf", "lm", "uv"):
        both[k] = np.concatenate([a[k], c[k]])
    for min_kf in (1, 3):
        ra = CR.compose(a, ida, None, [0, 5], min_kf, CR.oracle_run(oracle))
        rc = CR.compose(c, idc, None, [0, 4], min_kf, CR.oracle_run(oracle))
        rb = CR.compose(both, np.concatenate([ida, idc]), None, [0, 5, 9], min_kf, CR.oracle_run(oracle))
        assert np.array_equal(rb["T"], np.concatenate([ra["T"], rc["T"]])) and np.array_equal(rb["inl"], np.concatenate([ra["inl"], rc["inl"]]))
        assert np.array_equal(rb["ran"], np.concatenate([ra["ran"], rc["ran"]]))
        assert [s["n_windows"] for s in rb["steps"]] == [2, 2, 2, 2, 1] and rb["steps"][4]["windows"] == [4]
        assert rb["steps"][1]["windows"] == [1, 6]
        assert min_kf != 1 or ((ra["inl"] == 0).any() and (rc["inl"] == 0).any())
