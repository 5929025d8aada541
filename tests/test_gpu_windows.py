"""GPU parity of the device-side graph construction (vslam_build_windows_dev, track_kernels.hip) against oracle/windows.c, and of the
BA schedule on the windows it builds against the oracle's optimisers.  Reference: VO::insert_key_frame visual_odometry.cpp:363-424,
optimize_map optimization.cpp:127-214 (graph), :160 (landmark filter), optimize_pose_only :334 (its filter), run_vslam.cpp:58-71."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def _oracle_windows(oracle, pipe, out, n_kf, **caps):
    B = pipe.B
    return oracle.build_windows(out["kps"][:B], out["lr"], out["nlr"], out["xyz"], out["valid"], out["rel"], out["f2f"][:B - 1], out["nf2f"][:B - 1],
                                out["inl"][:B - 1], out["Tpnp"][:B - 1], n_kf=n_kf, **caps)


def test_track_rule_reference_vs_round5(oracle, synth):
    """[r6] the same front-end results under both track rules, device vs oracle each: the reference's rule (a match continues a track whenever its last-frame
    keypoint is a feature, visual_odometry.cpp:568-599) keeps every link of the old one (only matches out of a keypoint with its own depth) and adds links
    through keypoints the L/R match missed -- more observations per landmark, fewer landmarks created anew (with a third of the keypoints owning a depth
    the effect is a few per cent: 1.30 -> 1.33 observations per landmark on this sequence)"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 14, 10
    pipe = KeyframePipeline(B, anms_num=1500, n_kf=n_kf, unique_frames=B, seed=7, ba_windows="tracks")
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track()
        res = {}
        for rule in (0, 1):
            pipe.vo.set_tuning(track_rule=rule)
            pipe.stage_build_windows()
            out = pipe.download()
            w = _oracle_windows(oracle, pipe, out, n_kf, track_rule=rule)
            nl, ne = _compare(out, w, B)
            res[rule] = (nl, ne, np.diff(w["lm_off"]), np.diff(w["edge_off"]))
        pipe.vo.set_tuning(track_rule=-1)
        (nl0, ne0, l0, e0), (nl1, ne1, l1, e1) = res[0], res[1]
        assert ne1 > ne0 + 100 and nl1 < nl0 and (e1[1:] / l1[1:]).mean() > (e0[1:] / l0[1:]).mean() + 0.01, (ne0, ne1, nl0, nl1)
    finally:
        pipe.close()


def _compare(out, w, B):
    assert out["ba_build_status"][0] == w["status"]
    assert np.array_equal(out["ba_nkf"], w["n_kf"])
    assert np.array_equal(out["ba_lm_off"], w["lm_off"]) and np.array_equal(out["ba_e_off"], w["edge_off"])
    nl, ne = int(w["lm_off"][B]), int(w["edge_off"][B])
    assert np.array_equal(out["ba_kf"][:ne], w["kf_idx"][:ne]), "keyframe index of the edges"
    assert np.array_equal(out["ba_lm"][:ne], w["lm_idx"][:ne]), "landmark index of the edges"
    assert np.array_equal(out["ba_uv"][:ne], w["uv"][:ne]), "observations"
    assert np.array_equal(out["ba_rel"][:nl], w["reliable"][:nl]), "reliable_depth_"
    assert np.allclose(out["ba_xyz"][:nl], w["xyz"][:nl], rtol=2e-6, atol=1e-6), np.abs(out["ba_xyz"][:nl] - w["xyz"][:nl]).max()
    return nl, ne


@pytest.mark.parametrize("B,anms,n_kf,depth", [(13, 500, 10, "match"), (6, 1500, 4, "match"), (5, 500, 3, "sgbm")])
def test_build_windows_matches_oracle(oracle, synth, B, anms, n_kf, depth):
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    pipe = KeyframePipeline(B, anms_num=anms, n_kf=n_kf, unique_frames=B, seed=5, ba_windows="tracks", depth=depth)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        out = pipe.download()
        w = _oracle_windows(oracle, pipe, out, n_kf)
        nl, ne = _compare(out, w, B)
        assert w["status"] == 0 and (out["ba_inl"][:nl] == 1).all()
        assert np.allclose(out["ba_T"], w["T"], rtol=1e-9, atol=1e-12)
        # the map is a real one: windows slide, tracks are longer than one frame, both kinds of landmark exist
        per = np.diff(w["lm_off"]); per_e = np.diff(w["edge_off"])
        assert per.min() > 50 and (per_e[1:] > per[1:]).all() and per_e[0] == per[0] and w["n_kf"].max() == min(n_kf, B)
        assert 0 < w["reliable"][:nl].mean() < 1
        # poses really are the chained pose-stage estimates (forward motion of ~1 m per frame along z)
        assert abs(w["T"][B - 1, int(w["n_kf"][B - 1]) - 1, 6]) > 0.3 * (B - 1)
    finally:
        pipe.close()


def test_build_windows_capacity_overflow(oracle, synth):
    """arrays too small: the windows from the first that does not fit come out empty, the status word says so, nothing is written past the end"""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B = 6
    pipe = KeyframePipeline(B, anms_num=500, n_kf=4, unique_frames=B, seed=5, ba_windows="tracks", lm_per_window=200, edges_per_window=260)
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track()
        pipe.ba_kf.fill_(-7)
        pipe.stage_build_windows()
        out = pipe.download()
        w = _oracle_windows(oracle, pipe, out, 4, lm_capacity=pipe.lm_capacity, edge_capacity=pipe.edge_capacity)
        assert w["status"] == 1
        _, ne = _compare(out, w, B)
        assert (out["ba_kf"][ne:] == -7).all()
        assert 0 < ne < pipe.edge_capacity
    finally:
        pipe.close()


def test_ba_schedule_on_built_windows_matches_oracle(oracle, synth):
    """one step = one pipeline: the BA consumes the windows built from this step's own matches and poses.  Oracle composite per window:
    the schedule of run_vslam.cpp:58-71 with optimize_map's landmark filter is_inlier && reliable_depth_ (optimization.cpp:160) and
    optimize_pose_only's is_inlier (:334)."""
    from stereo_visual_slam_amd.pipeline import KeyframePipeline
    B, n_kf = 12, 10
    pipe = KeyframePipeline(B, anms_num=500, n_kf=n_kf, unique_frames=B, seed=6, ba_windows="tracks")
    try:
        pipe.stage_orb(); pipe.stage_stereo_match(); pipe.stage_track(); pipe.stage_build_windows()
        built = pipe.download()
        pipe.vo.ba_batch_dev(pipe.ba_batch, schedule=1)
        done = pipe.download()
        assert (pipe.vo.ba_status(B) == 0).all() and built["ba_build_status"][0] == 0
        lm_off, e_off = built["ba_lm_off"], built["ba_e_off"]
        for b in (0, 1, 4, 9, 11):
            nk = int(built["ba_nkf"][b])
            kf, lm, uv = (built[k][e_off[b]:e_off[b + 1]] for k in ("ba_kf", "ba_lm", "ba_uv"))
            xyz = built["ba_xyz"][lm_off[b]:lm_off[b + 1]]; rel = built["ba_rel"][lm_off[b]:lm_off[b + 1]].astype(bool)
            T = built["ba_T"][b][:nk].copy(); inl = np.ones(len(xyz), np.uint8)
            for iters, upd in ((5, False), (5, False), (10, True)):
                act = (inl.astype(bool) & rel)[lm]
                T2, _, chi2, _ = oracle.local_ba(T, xyz, kf[act], lm[act], uv[act], iters=iters)
                _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
                if upd:
                    T = T2
            act = inl.astype(bool)[lm]
            T2, chi2, _ = oracle.pose_only_window(T, xyz, kf[act], lm[act], uv[act], iters=10)
            _, inl, _, _ = oracle.chi2_classify(chi2, lm[act], inl)
            assert np.allclose(done["ba_T"][b][:nk], T2, rtol=1e-4, atol=1e-6), (b, np.abs(done["ba_T"][b][:nk] - T2).max())
            got = done["ba_inl"][lm_off[b]:lm_off[b + 1]]
            assert np.array_equal(got, inl), (b, int((got != inl).sum()))
            if nk > 1:
                assert not np.allclose(done["ba_T"][b][:nk], built["ba_T"][b][:nk], atol=1e-9)   # the BA moved the poses
    finally:
        pipe.close()


def _random_tracks(rng, F, cap, n_kp_max):
    """random front-end results with the invariants the real stages guarantee: an association list has distinct keypoints, a frame-to-frame
    match list is one-to-one (cross-checked), everything else -- counts, depth flags, inlier flags, poses -- is arbitrary"""
    import oracle as O
    kps = np.zeros((F, cap), O.KEYPOINT_DTYPE); nk = rng.integers(1, n_kp_max + 1, F)
    for f in range(F):
        kps["x"][f, :nk[f]] = rng.uniform(0, 1241, nk[f]).astype(np.float32); kps["y"][f, :nk[f]] = rng.uniform(0, 376, nk[f]).astype(np.float32)
    lr = np.zeros((F, cap), O.DMATCH_DTYPE); nlr = np.zeros(F, np.int32)
    xyz = rng.uniform(-20, 20, (F, cap, 3)).astype(np.float32); xyz[..., 2] = rng.uniform(5, 60, (F, cap)).astype(np.float32)
    valid = (rng.random((F, cap)) < rng.uniform(0.3, 0.95)).astype(np.uint8); rel = (rng.random((F, cap)) < rng.uniform(0.1, 0.9)).astype(np.uint8)
    for f in range(F):
        n = int(rng.integers(0, nk[f] + 1)); q = rng.permutation(nk[f])[:n]
        if rng.random() < 0.5:
            q = np.sort(q)
        lr["queryIdx"][f, :n] = q; lr["trainIdx"][f, :n] = rng.integers(0, cap, n); nlr[f] = n
    f2f = np.zeros((F - 1, cap), O.DMATCH_DTYPE); nf2f = np.zeros(F - 1, np.int32)
    for i in range(F - 1):
        n = int(rng.integers(0, min(nk[i], nk[i + 1]) + 1))
        f2f["queryIdx"][i, :n] = np.sort(rng.permutation(nk[i])[:n]); f2f["trainIdx"][i, :n] = rng.permutation(nk[i + 1])[:n]; nf2f[i] = n
    inl = (rng.random((F - 1, cap)) < rng.uniform(0.2, 1.0)).astype(np.uint8)
    T_rel = np.stack([O.se3_exp(np.concatenate([rng.normal(0, 0.3, 3), rng.normal(0, 0.02, 3)])) for _ in range(F - 1)]) if F > 1 else np.zeros((0, 7))
    return kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk.astype(np.int32)


@pytest.mark.parametrize("seed", range(6))
def test_build_windows_random_tracks_vs_oracle(pkg, oracle, seed):
    """the builder alone, on random association / match / flag tables (chains of every length, unreliable -> reliable updates mid-chain,
    dropped links, empty frames, n_kf from 1 to 12, capacity overflow), through vslam_build_windows_dev against oracle/windows.c"""
    _random_tracks_vs_oracle(pkg, oracle, seed)


def _random_tracks_vs_oracle(pkg, oracle, seed, thrs=(4.0, 300.0, 1200.0), cam=None):
    """cam (fx, fy, cx, cy, b): the contexts' camera, its K handed to the oracle (None: the KITTI camera of both).  Returns the number of edges by
    which the oracle's windows under that camera differ from its windows under the KITTI camera, summed over the cases."""
    import torch
    rng = np.random.default_rng(1000 + seed)
    K = None if cam is None else np.asarray(cam, np.float64)[:4]
    kw = {} if cam is None else dict(cam=cam)
    n_camera_edges = 0
    # [r6] the track rule: seeds 0-3 the reference's (a match continues a track whenever its last-frame keypoint is a feature; one without a depth is judged by
    # reprojecting the landmark's map position), seeds 4-5 the convention of rounds 4-5.  Random geometry rarely reprojects within the product's 4 px, so
    # the cases also run with thresholds of hundreds of pixels: then many depth-less links hold, chains of them, with position updates in between.
    rule = 1 if seed < 4 else 0
    ctxs = {thr: pkg.VO(device=0, max_batch=1, pnp_reproj_thr=thr, **kw) for thr in thrs}
    for c_ in ctxs.values():
        c_.set_tuning(track_rule=rule)
    n_depthless_links = 0
    try:
        for case in range(12):
            thr = thrs[case % len(thrs)]; ctx = ctxs[thr]
            F = int(rng.integers(1, 40)); cap = int(rng.choice([64, 100, 256])); n_kf = int(rng.integers(1, 13))
            kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, nk = _random_tracks(rng, F, cap, int(rng.integers(1, cap + 1)))
            full = oracle.build_windows(kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, n_kf=n_kf, lm_capacity=F * cap * (n_kf + 1),
                                        edge_capacity=2 * F * cap * (n_kf + 1), reproj_thr=thr, track_rule=rule, K=K)   # (a landmark is in up to n_kf windows)
            if K is not None:
                kitti = oracle.build_windows(kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, n_kf=n_kf, lm_capacity=F * cap * (n_kf + 1),
                                             edge_capacity=2 * F * cap * (n_kf + 1), reproj_thr=thr, track_rule=rule)
                n_camera_edges += abs(int(full["edge_off"][F]) - int(kitti["edge_off"][F]))
            if rule:
                old = oracle.build_windows(kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, n_kf=n_kf, lm_capacity=F * cap * (n_kf + 1),
                                           edge_capacity=2 * F * cap * (n_kf + 1), track_rule=0)
                n_depthless_links += int(full["edge_off"][F]) - int(old["edge_off"][F])   # (with n_kf = 1 a link adds no edge: edges minus landmarks stays 0)
            assert full["status"] == 0
            nl_tot, ne_tot = int(full["lm_off"][F]), int(full["edge_off"][F])
            shrink = rng.random() < 0.3 and nl_tot > 4
            lm_cap = max(int(nl_tot * rng.uniform(0.3, 0.9)), 1) if shrink else nl_tot + 7
            e_cap = ne_tot + 5
            w = oracle.build_windows(kps, lr, nlr, xyz, valid, rel, f2f, nf2f, inl, T_rel, n_kf=n_kf, lm_capacity=lm_cap, edge_capacity=e_cap, reproj_thr=thr,
                                     track_rule=rule, K=K)
            d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            t_kps, t_lr, t_nlr, t_xyz, t_valid, t_rel, t_nk = d(kps.view(np.uint8)), d(lr.view(np.uint8)), d(nlr), d(xyz), d(valid), d(rel), d(nk)
            t_f2f = d(f2f.view(np.uint8)) if F > 1 else torch.zeros(16, dtype=torch.uint8, device="cuda")
            t_nf2f = d(nf2f) if F > 1 else torch.zeros(1, dtype=torch.int32, device="cuda")
            t_inl = d(inl) if F > 1 else torch.zeros(1, dtype=torch.uint8, device="cuda")
            t_T = d(T_rel) if F > 1 else torch.zeros(7, dtype=torch.float64, device="cuda")
            tr = pkg.TracksIn()
            tr.n_frames = F; tr.kp_capacity = cap; tr.lr_capacity = cap; tr.match_capacity = cap; tr.pnp_capacity = cap
            tr.d_kps = t_kps.data_ptr(); tr.d_lr = t_lr.data_ptr(); tr.d_nlr = t_nlr.data_ptr(); tr.d_xyz = t_xyz.data_ptr(); tr.d_valid = t_valid.data_ptr()
            tr.d_reliable = t_rel.data_ptr(); tr.d_f2f = t_f2f.data_ptr(); tr.d_nf2f = t_nf2f.data_ptr(); tr.d_pose_inlier = t_inl.data_ptr()
            tr.d_T_rel = t_T.data_ptr(); tr.d_nkps = t_nk.data_ptr() if case % 2 == 0 else None
            o = dict(lm_off=torch.zeros(F + 1, dtype=torch.int32, device="cuda"), e_off=torch.zeros(F + 1, dtype=torch.int32, device="cuda"),
                     nkf=torch.zeros(F, dtype=torch.int32, device="cuda"), T=torch.zeros((F, n_kf, 7), dtype=torch.float64, device="cuda"),
                     xyz=torch.zeros((lm_cap, 3), dtype=torch.float32, device="cuda"), rel=torch.zeros(lm_cap, dtype=torch.uint8, device="cuda"),
                     inl=torch.zeros(lm_cap, dtype=torch.uint8, device="cuda"), kf=torch.full((e_cap,), -7, dtype=torch.int32, device="cuda"),
                     lm=torch.zeros(e_cap, dtype=torch.int32, device="cuda"), uv=torch.zeros((e_cap, 2), dtype=torch.float32, device="cuda"),
                     st=torch.zeros(1, dtype=torch.int32, device="cuda"))
            bb = pkg.BaBatch()
            bb.d_lm_off = o["lm_off"].data_ptr(); bb.d_edge_off = o["e_off"].data_ptr(); bb.d_T_c_w = o["T"].data_ptr(); bb.d_xyz = o["xyz"].data_ptr()
            bb.d_reliable = o["rel"].data_ptr(); bb.d_lm_inlier = o["inl"].data_ptr(); bb.d_kf_idx = o["kf"].data_ptr(); bb.d_lm_idx = o["lm"].data_ptr()
            bb.d_uv = o["uv"].data_ptr(); bb.d_n_kf = o["nkf"].data_ptr()
            torch.cuda.synchronize()
            ctx.build_windows_dev(tr, n_kf, lm_cap, e_cap, bb, o["st"].data_ptr())
            ctx.sync()
            g = {k: v.cpu().numpy() for k, v in o.items()}
            tag = (seed, case, F, cap, n_kf, shrink)
            assert g["st"][0] == w["status"] and (w["status"] == 1) == (shrink and lm_cap < nl_tot), tag
            assert np.array_equal(g["lm_off"], w["lm_off"]) and np.array_equal(g["e_off"], w["edge_off"]) and np.array_equal(g["nkf"], w["n_kf"]), tag
            nl, ne = int(w["lm_off"][F]), int(w["edge_off"][F])
            assert np.array_equal(g["kf"][:ne], w["kf_idx"][:ne]) and np.array_equal(g["lm"][:ne], w["lm_idx"][:ne]) and np.array_equal(g["uv"][:ne], w["uv"][:ne]), tag
            assert (g["kf"][ne:] == -7).all(), tag
            assert np.array_equal(g["rel"][:nl], w["reliable"][:nl]) and (g["inl"][:nl] == 1).all(), tag
            assert np.allclose(g["xyz"][:nl], w["xyz"][:nl], rtol=3e-6, atol=2e-5), (tag, np.abs(g["xyz"][:nl] - w["xyz"][:nl]).max())
            assert np.allclose(g["T"], w["T"], rtol=1e-9, atol=1e-11), tag
            assert bb.n_windows == F and bb.n_kf == n_kf and bb.total_lm == lm_cap and bb.total_edge == e_cap
        assert rule == 0 or n_depthless_links != 0, "the random cases never exercised a link through a keypoint without depth"
    finally:
        for c_ in ctxs.values():
            c_.close()
    return n_camera_edges
