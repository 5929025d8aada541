"""GPU parity on the tie-dense inputs of tests/structured_inputs.py: ORB selection, ANMS, orientation + rBRIEF, the matcher and SGBM against the CPU
oracle where a tie rule decides the result -- ties kept at the FAST-score and Harris cuts of orb_select_kernel, the stable (response, input index)
order and the radius ties of orb_anms_kernel, "the first minimum over d wins" in the SGBM winner -- and the capacity contract of the ORB kernels:
an input that exceeds a device capacity ends in the capacity error (host tier) / a status bit (device tier), never in a truncated keypoint set.
tests/test_structured_inputs.py shows on the CPU that the inputs have the ties and cross the capacities they are named for.  Everything is bit-exact."""
import numpy as np
import pytest

import structured_inputs as S

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
FUSE = {"fused": 1, "separate": 1000000}          # orb_fuse_min: orb_pyrblur_kernel (FAST inside the tile pass) or the separate resize / FAST / blur kernels
SGBM_MODES = {"fused-slab64": (1, 64), "fused-slab32": (1, 32), "separate": (1000000, 64)}


def _kps_equal(a, b, what=""):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in FIELDS:
        bad = np.nonzero(a[f] != b[f])[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:5], a[f][bad[:5]], b[f][bad[:5]])


@pytest.fixture(scope="module")
def ref(oracle):
    """oracle results, once per module: {case: dict(img, det, fd={anms_num: (kps, desc)})}"""
    out = {}
    for c in S.ORB_CASES:
        img = S.make(c)
        out[c["name"]] = dict(img=img, det=oracle.orb_detect(img, c["nfeatures"]),
                              fd={num: oracle.feature_detection(img, c["nfeatures"], num) for num in (500, 1500)})
    return out


def _groups():
    g = {}
    for c in S.ORB_CASES:
        g.setdefault((c["size"], c["nfeatures"]), []).append(c)
    return g


def _ctx(pkg, size, nfeatures, anms_num, fuse="separate", **kw):
    ctx = pkg.VO(device=0, img_w=size[1], img_h=size[0], orb_nfeatures=nfeatures, anms_num=anms_num, **kw)
    ctx.set_tuning(orb_fuse_min=FUSE[fuse])
    return ctx


# ------------------------------------------------------------------------------------------------ ORB, host tier
@pytest.mark.parametrize("fuse", list(FUSE))
@pytest.mark.parametrize("anms_num", [500, 1500])
def test_orb_host_tier_on_every_case(pkg, oracle, ref, anms_num, fuse):
    """orb_detect, adaptive_non_maximal_suppresion, orb_compute and feature_detection on every in-capacity case: every keypoint field and every
    descriptor byte equals the oracle's, on the fused and on the separate kernels"""
    for (size, nf), cases in _groups().items():
        ctx = _ctx(pkg, size, nf, anms_num, fuse, max_batch=1)
        try:
            for c in cases:
                r = ref[c["name"]]
                _kps_equal(ctx.orb_detect(r["img"]), r["det"], c["name"] + " detect")
                kept = oracle.anms(r["det"], anms_num)
                _kps_equal(ctx.adaptive_non_maximal_suppresion(r["det"], anms_num), kept, c["name"] + " anms")
                gk, gd = ctx.orb_compute(r["img"], kept)
                wk, wd = oracle.orb_compute(r["img"], kept)
                _kps_equal(gk, wk, c["name"] + " compute")
                assert np.array_equal(gd, wd), (c["name"], "compute", int((gd != wd).any(axis=1).sum()))
                gk, gd = ctx.feature_detection(r["img"])
                wk, wd = r["fd"][anms_num]
                _kps_equal(gk, wk, c["name"] + " feature_detection")
                assert gd.shape == wd.shape and np.array_equal(gd, wd), (c["name"], "descriptors", int((gd != wd).any(axis=1).sum()))
        finally:
            ctx.close()


@pytest.mark.parametrize("name", ["tile20", "tile32", "mirror", "checker8", "blobs"])
def test_anms_num_around_radius_ties(vo, oracle, ref, name):
    """num inside a group of equal radii, just above and just below it (found on the CPU from the radii), and the degenerate values of test_anms_parity"""
    kps = ref[name]["det"]
    ties = S.anms_tie_nums(kps)
    assert ties
    for num in [n for n, _ in ties] + [500, 1500, len(kps), len(kps) + 1, 1]:
        _kps_equal(vo.adaptive_non_maximal_suppresion(kps, num), oracle.anms(kps, num), "%s num %d" % (name, num))
    for num, want in ties:
        assert len(vo.adaptive_non_maximal_suppresion(kps, num)) == want


@pytest.mark.parametrize("n,groups", [(2000, 1), (3000, 1), (2000, 4), (3000, 3), (4096, 5)])
def test_anms_user_keypoints_with_tied_responses(vo, oracle, n, groups):
    """user-supplied keypoints on a lattice, all responses equal or in a few tied groups, in shuffled input order: the output ORDER is the oracle's
    (stable by input index inside a tie), through every tie group of the radii"""
    kps = S.tied_keypoints(n, groups, seed=n + groups)
    nums = [1, 100, 500, 1500, n] + [m for m, _ in S.anms_tie_nums(kps)]
    for num in nums:
        _kps_equal(vo.adaptive_non_maximal_suppresion(kps, num), oracle.anms(kps, num), "n %d groups %d num %d" % (n, groups, num))
    neg = kps.copy(); neg["response"] = -neg["response"]      # 1.11 x a negative response is smaller: equal responses suppress each other, in input order
    for num in (100, 500):
        _kps_equal(vo.adaptive_non_maximal_suppresion(neg, num), oracle.anms(neg, num), "negative, num %d" % num)


@pytest.mark.parametrize("fuse", list(FUSE))
def test_orb_compute_on_flat_and_symmetric_patches(pkg, oracle, fuse):
    """descriptors of user keypoints on a constant image (all bits 0), on step edges, on checkerboard crossings and on blob centres, octaves 0..3, angles
    at multiples of 45 degrees: comparisons of EQUAL pixels (a < b is false both ways) and pattern points that round onto the same pixel"""
    ctx = _ctx(pkg, S.ODD, 1000, 500, fuse, max_batch=1)
    try:
        for i, (img, kps) in enumerate(S.flat_and_symmetric_keypoints()):
            gk, gd = ctx.orb_compute(img, kps)
            wk, wd = oracle.orb_compute(img, kps)
            _kps_equal(gk, wk, "image %d" % i)
            assert np.array_equal(gd, wd), i
            if i == 0:
                assert len(gd) == len(kps) and not gd.any()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ ORB, device tier
def _run_dev(ctx, images, pad=64):
    import torch
    from stereo_visual_slam_amd import KEYPOINT_DTYPE
    B = len(images); h, w = images[0].shape; pitch = (w + 63) // 64 * 64 + pad
    buf = np.zeros((B, h, pitch), np.uint8)
    for b, im in enumerate(images):
        buf[b, :, :w] = im
    dev = torch.device("cuda:0")
    d_img = torch.from_numpy(buf).to(dev)
    cap = ctx.params.kp_capacity
    d_kps = torch.zeros((B, cap, 28), dtype=torch.uint8, device=dev); d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.feature_detection_dev(d_img.data_ptr(), h * pitch, pitch, B, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr())
    ctx.sync()
    st = ctx.orb_status(B)
    cnt = d_cnt.cpu().numpy(); kk = d_kps.cpu().numpy(); dd = d_desc.cpu().numpy()
    return st, cnt, [kk[b].reshape(-1).view(KEYPOINT_DTYPE)[:cnt[b]] for b in range(B)], [dd[b][:cnt[b]] for b in range(B)]


@pytest.mark.parametrize("fuse", list(FUSE))
def test_device_tier_mixed_batch(pkg, oracle, synth, ref, fuse):
    """one feature_detection_dev call over structured cases mixed with a noise image, rows padded beyond the 64-byte pitch: status 0, counts, keypoints and
    descriptors per item"""
    names = ["tile20", "mirror", "checker8", "blobs", "steps", "tile97", "binary3", "tile32"]
    images = [ref[n]["img"] for n in names[:3]] + [synth.noise_image(0)] + [ref[n]["img"] for n in names[3:]]
    want = [ref[n]["fd"][500] for n in names[:3]] + [oracle.feature_detection(images[3], 3000, 500)] + [ref[n]["fd"][500] for n in names[3:]]
    ctx = _ctx(pkg, S.KITTI, 3000, 500, fuse, max_batch=len(images))
    try:
        st, cnt, kps, desc = _run_dev(ctx, images)
        assert (st == 0).all(), st
        for b, (wk, wd) in enumerate(want):
            assert cnt[b] == len(wk), (b, cnt[b], len(wk))
            _kps_equal(kps[b], wk, "item %d" % b)
            assert np.array_equal(desc[b], wd), b
    finally:
        ctx.close()


@pytest.mark.parametrize("fuse", list(FUSE))
@pytest.mark.parametrize("name", ["tile20", "mirror"])
def test_run_twice_is_bit_identical(pkg, ref, name, fuse):
    """arrival order (atomics in the candidate and survivor compaction, the ANMS cell lists) is nondeterministic exactly where ties live: the same call
    twice gives the same bytes, on the host tier, in ANMS alone and on the device tier with the case in every slot of a batch"""
    r = ref[name]
    ctx = _ctx(pkg, S.KITTI, 3000, 500, fuse, max_batch=4)
    try:
        a = ctx.feature_detection(r["img"]); b = ctx.feature_detection(r["img"])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        for num in (500, 1500):
            x = ctx.adaptive_non_maximal_suppresion(r["det"], num); y = ctx.adaptive_non_maximal_suppresion(r["det"], num)
            assert x.tobytes() == y.tobytes()
        s1, c1, k1, d1 = _run_dev(ctx, [r["img"]] * 4); s2, c2, k2, d2 = _run_dev(ctx, [r["img"]] * 4)
        assert (s1 == 0).all() and (s2 == 0).all() and np.array_equal(c1, c2)
        for i in range(4):
            assert k1[i].tobytes() == k2[i].tobytes() == k1[0].tobytes() == a[0].tobytes() and d1[i].tobytes() == d2[i].tobytes() == a[1].tobytes()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ ORB capacity contract
# in-capacity companions of the overflowing item in its batch, per context parameters (checked against the oracle's counts in the test)
COMPANIONS = {"tile12": ("noise", "tile32"), "tile16": ("noise", "tile32"), "binary2": ("noise", "tile20"), "blocky3600": ("checker8", "checker31"),
              "blocky9600": ("blobs", "steps"), "mirror_odd_cap256": ("blobs_odd", "ramp_odd")}


def _companion(name, synth):
    if name == "noise":
        return synth.noise_image(0)
    if name == "ramp_odd":
        return S.linear_ramp(*S.ODD)
    return S.make(S.CASE[name])


@pytest.mark.parametrize("fuse", list(FUSE))
@pytest.mark.parametrize("case", S.OVERFLOW_CASES, ids=lambda c: c["name"])
def test_capacity_overflow_is_an_error_not_a_truncated_set(pkg, oracle, synth, case, fuse):
    """kStCandOverflow (2), kStSelOverflow (4), kStAnmsOverflow (8) and kStOutOverflow (16), each reached with an input whose oracle counts cross that limit
    (tests/test_structured_inputs.py::test_overflow_cases_cross_the_limit_they_are_meant_to_cross): the host tier raises VslamError naming the capacity; the
    device tier sets the expected bit -- and no bit that the oracle's counts rule out -- on that item, and the other items of the same batch stay bit-exact
    with status 0.  vslam_create accepts every parameter these cases need (orb_nfeatures 3600 / 9600, kp_capacity 256)."""
    img = S.make(case)
    nf, num, cap = case["nfeatures"], case["anms_num"], case["kp_capacity"]
    others = [_companion(n, synth) for n in COMPANIONS[case["name"]]]
    for o in others:
        bits, cnt = S.device_capacity_bits(oracle, o, nf, num, cap)
        assert bits == 0 and cnt["unknown"] == 0, cnt
    ctx = _ctx(pkg, case["size"], nf, num, fuse, max_batch=3, kp_capacity=cap)
    try:
        with pytest.raises(pkg.VslamError) as e:
            ctx.feature_detection(img)
        assert "capacity" in str(e.value).lower()
        st, cnt, kps, desc = _run_dev(ctx, [others[0], img, others[1]])
        print(case["name"], "status", st, "counts", cnt)
        assert st[1] & case["bits"] == case["bits"] and st[1] & ~(case["bits"] | case["may"]) == 0, st
        assert st[0] == 0 and st[2] == 0, st
        for b, o in ((0, others[0]), (2, others[1])):
            wk, wd = oracle.feature_detection(o, nf, num)
            _kps_equal(kps[b], wk, "item %d" % b)
            assert np.array_equal(desc[b], wd), b
        gk, gd = ctx.feature_detection(others[0])            # and the context is usable after the error
        _kps_equal(gk, oracle.feature_detection(others[0], nf, num)[0], "after the error")
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ matcher, end to end
def test_matcher_on_descriptors_of_a_tiled_frame(pkg, vo, oracle, ref):
    """descriptors of a tiled frame and of the same frame shifted by 7 px: many rows are byte-identical (S.MATCHER_TILED records the oracle's count and
    the floor, half of it), so distance ties are everywhere; feature_matching with the gate on and off against the oracle"""
    M = S.MATCHER_TILED
    img = ref[M["case"]]["img"]
    ctx = _ctx(pkg, S.KITTI, 3000, M["anms_num"], max_batch=1)
    try:
        k0, d0 = ctx.feature_detection(img); k1, d1 = ctx.feature_detection(np.roll(img, M["shift"], axis=1))
    finally:
        ctx.close()
    assert np.array_equal(d0, ref[M["case"]]["fd"][M["anms_num"]][1])
    dup = S.duplicate_rows(d0)
    print("duplicate descriptor rows", dup, "of", len(d0))
    assert dup >= M["floor"]
    for q, t in ((d0, d1), (d1, d0), (d0, d0)):
        for gate in (False, True):
            g = vo.feature_matching(q, t, 1.0, gate=gate)
            w = oracle.feature_matching(q, t, 1.0) if gate else oracle.bf_match_xcheck(q, t)
            assert len(g) == len(w) and all(np.array_equal(g[f], w[f]) for f in ("queryIdx", "trainIdx", "distance")), (gate, len(g), len(w))


# ------------------------------------------------------------------------------------------------ SGBM
@pytest.fixture(params=list(SGBM_MODES))
def sgbm_ctx(request, pkg):
    """a context with the SGBM kernel choice forced: the fused top-down + forward kernels with 64-row or 32-row slabs, or the separate kernels"""
    fuse, rows = SGBM_MODES[request.param]
    ctx = pkg.VO(device=0, max_batch=6)
    ctx.set_tuning(sgbm_fuse_min=fuse, sgbm_fwd_min=fuse, sgbm_fw_rows=rows)
    yield ctx
    ctx.close()


def _sgbm_check(ctx, oracle, L, R, answer=None):
    gf, gi, graw = ctx.disparity_map(L, R, return_i16=True)
    wi, wraw = oracle.sgbm_compute(L, R, return_raw=True)
    assert np.array_equal(graw, wraw), "raw SGBM differs at %d px" % (graw != wraw).sum()      # the winners themselves, before the median / speckle filters
    assert np.array_equal(gi, wi), "filtered map differs at %d px" % (gi != wi).sum()
    assert np.array_equal(gf, oracle.disparity_map(L, R))
    if answer is not None:
        assert (gf[:, :96] == -1).all() and (gf[:, 96:] == float(answer)).all(), np.unique(gf[:, 96:], return_counts=True)
    return gi


def test_sgbm_periodic_pairs_known_answer(sgbm_ctx, oracle):
    """noise-free periodic pairs: exact cost ties at d, d + p, d + 2p; the disparity equals the oracle's and shift mod period, the FIRST minimum"""
    for k, pair in enumerate(S.SGBM_CLEAN):
        w, h = S.KNOWN_ANSWER_SIZES[k % 2]
        L, R = S.periodic_pair(w=w, h=h, **pair)
        _sgbm_check(sgbm_ctx, oracle, L, R, pair["shift"] % pair["period"])


def test_sgbm_noisy_periodic_pairs(sgbm_ctx, oracle):
    """+- 2..4 grey levels on the right image: near-ties between the disparities of one residue class, which the uniqueness and left-right checks judge"""
    for pair in S.SGBM_NOISY:
        L, R = S.periodic_pair(pair["period"], pair["shift"], pair["noise"])
        gi = _sgbm_check(sgbm_ctx, oracle, L, R)
        share = S.sgbm_winner_shares(gi)
        for d, fig in pair["winners"].items():
            assert share.get(d, 0.0) >= fig["floor"], (d, share.get(d), fig)


def test_sgbm_kitti_sized_periodic_pairs(sgbm_ctx, oracle):
    k = S.KITTI_PERIODIC
    L, R = S.periodic_pair(shift=37, **k)
    _sgbm_check(sgbm_ctx, oracle, L, R, 37 % k["period"])
    L, R = S.periodic_pair(shift=37, noise=3, **k)
    gi = _sgbm_check(sgbm_ctx, oracle, L, R)
    assert len([d for d, s in S.sgbm_winner_shares(gi).items() if s > 0.05 and d % k["period"] == 5]) >= 2


def test_sgbm_periodic_pairs_batched_dev(sgbm_ctx, oracle):
    """disparity_map_dev on a batch that mixes noise-free and noisy periodic pairs (padded pitch): the f32 map, the CV_16S map and the raw winners per item"""
    import torch
    w, h, pitch = 385, 120, 448
    specs = [dict(period=32, shift=5), dict(period=24, shift=67), dict(period=32, shift=5, noise=3), dict(period=64, shift=70), dict(period=64, shift=70, noise=2),
             dict(period=48, shift=40)]
    pairs = [S.periodic_pair(w=w, h=h, **s) for s in specs]
    B = len(pairs)
    buf = np.zeros((2, B, h, pitch), np.uint8)
    for b, (L, R) in enumerate(pairs):
        buf[0, b, :, :w] = L; buf[1, b, :, :w] = R
    d = torch.from_numpy(buf).cuda()
    out = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
    i16 = torch.empty((B, h, w), dtype=torch.int16, device="cuda"); raw = torch.empty((B, h, w), dtype=torch.int16, device="cuda")
    sgbm_ctx.disparity_map_dev(d[0].data_ptr(), d[1].data_ptr(), h * pitch, pitch, w, h, B, out.data_ptr(), i16.data_ptr(), raw.data_ptr())
    sgbm_ctx.sync()
    gf, gi, graw = out.cpu().numpy(), i16.cpu().numpy(), raw.cpu().numpy()
    for b, ((L, R), s) in enumerate(zip(pairs, specs)):
        wi, wraw = oracle.sgbm_compute(L, R, return_raw=True)
        assert np.array_equal(graw[b], wraw) and np.array_equal(gi[b], wi) and np.array_equal(gf[b], oracle.disparity_map(L, R)), b
        if not s.get("noise"):
            assert (gf[b][:, 96:] == float(s["shift"] % s["period"])).all() and (gf[b][:, :96] == -1).all(), b
