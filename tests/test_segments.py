"""CPU: the numpy side of segmented batches (several independent sequences in one batch) -- trajectory.assemble_trajectories against
assemble_trajectory per segment, and the split / concat helpers of the GPU tests against oracle/windows.c on a single segment."""
import numpy as np
import pytest

from segments_ref import concat_windows, split_tables


def _culled_sets(rng, n, n_kf):
    """keyframe sets of n steps with an arbitrary member evicted once the set is full (what the culling may do), local frame ids"""
    kf = np.full((n, n_kf), -1, np.int32); ev = np.full(n, -1, np.int32)
    S = []
    for b in range(n):
        S.append(b)
        if len(S) > n_kf:
            ev[b] = S.pop(int(rng.integers(0, len(S) - 1)))
        kf[b, :len(S)] = S
    return kf, ev


def _gated_sets(rng, n, n_kf, state):
    """the same with a keyframe gate: only a state-2 step inserts; the sets repeat at the other steps"""
    kf = np.full((n, n_kf), -1, np.int32); ev = np.full(n, -1, np.int32)
    S = []
    for b in range(n):
        if state[b] == 2:
            S.append(b)
            if len(S) > n_kf:
                ev[b] = S.pop(0)
        kf[b, :len(S)] = S
    return kf, ev


def test_assemble_trajectories_equals_per_segment():
    from stereo_visual_slam_amd.trajectory import assemble_trajectories, assemble_trajectory
    rng = np.random.default_rng(3)
    n_kf = 4
    lens = [9, 1, 14, 2]
    state = [None, None, np.array([2, 2, 1, 0, 2, 2, 1, 2, 2, 0, 2, 2, 2, 1]), None]   # segment 2 is gated: invalid windows
    first = np.concatenate([[0], np.cumsum(lens)])
    kfs, evs, valids = [], [], []
    for n, st in zip(lens, state):
        kf, ev = _culled_sets(rng, n, n_kf) if st is None else _gated_sets(rng, n, n_kf, st)
        kfs.append(kf); evs.append(ev); valids.append(np.ones(n, bool) if st is None else st == 2)
    ba_T = rng.normal(size=(first[-1], n_kf, 7))
    reb = lambda a, lo: np.where(a >= 0, a + lo, -1)
    kf_all = np.concatenate([reb(k, lo) for k, lo in zip(kfs, first)]); ev_all = np.concatenate([reb(e, lo) for e, lo in zip(evs, first)])
    valid_all = np.concatenate(valids)
    got = assemble_trajectories(kf_all, ev_all, ba_T, first, valid_all)
    assert len(got) == len(lens)
    for s, (ids, T) in enumerate(got):
        lo, hi = first[s], first[s + 1]
        want_ids, want_T = assemble_trajectory(kfs[s], evs[s], ba_T[lo:hi], valids[s])
        assert np.array_equal(ids, want_ids) and np.array_equal(T, want_T), s
    assert np.array_equal(got[1][0], [0]) and len(got[2][0]) == int((state[2] == 2).sum())   # the one-frame segment; keyframes only under the gate
    # without window_valid every window counts (ungated segments only)
    got2 = assemble_trajectories(kf_all[:10], ev_all[:10], ba_T[:10], first[:3])
    assert np.array_equal(got2[0][0], got[0][0]) and np.array_equal(got2[0][1], got[0][1])
    # a set that reaches into another segment, and a malformed table, are refused
    bad = kf_all.copy(); bad[first[2], 1] = 0
    with pytest.raises(ValueError):
        assemble_trajectories(bad, ev_all, ba_T, first, valid_all)
    for f in ([0, 5], [1, 26], [0, 9, 9, 26]):
        with pytest.raises(ValueError):
            assemble_trajectories(kf_all, ev_all, ba_T, f, valid_all)


def test_split_concat_identity_on_one_segment(oracle):
    """concat_windows(split_tables(...)) with first = [0, F] is the identity against oracle.build_windows; on two segments the helpers cut the
    pair between them out and rebase the second segment's offsets"""
    from test_gpu_windows import _random_tracks
    rng = np.random.default_rng(11)
    F, cap, n_kf = 9, 64, 4
    kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = _random_tracks(rng, F, cap, 40)
    tabs = dict(kps=kps, lr=lr, nlr=nlr, xyz=xyz, valid=valid, rel=rel, f2f=f2f, nf2f=nf2f, inl=inl, T_rel=T_rel)
    build = lambda t: oracle.build_windows(t["kps"], t["lr"], t["nlr"], t["xyz"], t["valid"], t["rel"], t["f2f"], t["nf2f"], t["inl"], t["T_rel"], n_kf=n_kf,
                                           reproj_thr=300.0)
    whole = build(tabs)
    one = concat_windows([build(s) for s in split_tables(tabs, [0, F])])
    nl, ne = int(whole["lm_off"][F]), int(whole["edge_off"][F])
    assert ne > nl > 0 and one["status"] == whole["status"]
    for k in ("lm_off", "edge_off", "n_kf", "T"):
        assert np.array_equal(one[k], whole[k]), k
    for k, n in (("xyz", nl), ("reliable", nl), ("lm_inlier", nl), ("kf_idx", ne), ("lm_idx", ne), ("uv", ne)):
        assert np.array_equal(one[k], whole[k][:n]), k
    parts = split_tables(tabs, [0, 4, F])
    assert [len(p["kps"]) for p in parts] == [4, 5] and [len(p["f2f"]) for p in parts] == [3, 4]
    assert np.array_equal(parts[1]["f2f"], f2f[4:]) and np.array_equal(parts[0]["T_rel"], T_rel[:3])
    two = concat_windows([build(p) for p in parts])
    assert len(two["lm_off"]) == F + 1 and two["lm_off"][4] == build(parts[0])["lm_off"][4] and (np.diff(two["lm_off"]) >= 0).all()
    assert np.array_equal(two["n_kf"], [1, 2, 3, 4, 1, 2, 3, 4, 4])
    with pytest.raises(ValueError):
        split_tables(dict(a=np.zeros(F + 1)), [0, F])
