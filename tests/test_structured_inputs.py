"""CPU tests of the tie-dense inputs of tests/structured_inputs.py.

(a) teeth: the oracle's own output on every ORB case shows the ties the case is named for (the table's floors), and the overflow cases cross
    exactly the device capacities they are meant to cross;
(b) the oracle against the independent numpy restatements of tests/orb_restatements.py ON these inputs -- ANMS with tied responses and tied
    radii, retainBest at a cut with ties, Harris on tied pairs, FAST, rBRIEF on flat and symmetric patches, the orientation on zero moments;
(c) SGBM known answers: a noise-free horizontally periodic pair comes out as shift mod period at every evaluated pixel, which rests on
    "the first minimum over d wins" alone; noisy pairs split between winners of one residue class.
The GPU side (tests/test_gpu_ties.py) compares the kernels with the oracle on the same inputs."""
import numpy as np
import pytest

import orb_restatements as N
import structured_inputs as S

NUMS = (500, 1500)


@pytest.fixture(scope="module")
def detected(oracle):
    """{case name: (image, oracle keypoints)}"""
    out = {}
    for c in S.ORB_CASES:
        img = S.make(c)
        out[c["name"]] = (img, oracle.orb_detect(img, c["nfeatures"]))
    return out


# ------------------------------------------------------------------------------------------------ (a) teeth
def test_sizes_cover_kitti_and_the_odd_sizes():
    sizes = {c["size"] for c in S.ORB_CASES}
    assert {(376, 1241), (257, 333), (200, 1324)} <= sizes


@pytest.mark.parametrize("case", S.ORB_CASES, ids=lambda c: c["name"])
def test_case_has_the_ties_it_is_named_for(oracle, case):
    fig = S.tie_figures(oracle, S.make(case), case["nfeatures"], NUMS)
    print(case["name"], fig)
    for k, floor in case["floor"].items():
        assert fig[k] >= floor > 0, (k, fig[k], floor)
    assert case["floor"] == {k: v // 2 for k, v in case["oracle"].items() if k != "n" and v // 2 > 0}   # a floor is half of the recorded figure


@pytest.mark.parametrize("case", S.ORB_CASES, ids=lambda c: c["name"])
def test_table_figures_are_current(oracle, case):
    """the `oracle` column is what the oracle gives today (a changed generator or oracle shows up here with the fresh numbers, not as a silently toothless case)"""
    assert S.tie_figures(oracle, S.make(case), case["nfeatures"], NUMS) == case["oracle"]


def test_the_set_of_cases_covers_every_tie_rule():
    fl = {c["name"]: c["floor"] for c in S.ORB_CASES}
    assert sum("dup" in f for f in fl.values()) >= 8                          # tied responses: the stable sort of ANMS
    assert sum("over" in f for f in fl.values()) >= 6                         # a level above its quota: ties kept at a retainBest cut
    for num in NUMS:                                                          # ties kept at the num-th radius, both values of num
        assert any("anms%d" % num in f for f in fl.values()), num
    assert sum(any("anms%d" % num in f for num in NUMS) for f in fl.values()) >= 2
    assert sum("angle0" in f for f in fl.values()) >= 1                       # angle == 0 exactly (zero moment m01)
    assert any(c["oracle"]["n"] == 0 for c in S.ORB_CASES)                    # and images without a corner


def test_quotas_come_from_the_layout(oracle, detected):
    """`over` counts against the oracle's layout: on the cut cases at least one level holds MORE keypoints than its quota, and every keypoint above
    the quota shares its response with the weakest one kept at the quota (that is what "ties at the cut" means)"""
    seen = 0
    for c in S.ORB_CASES:
        if "over" not in c["floor"]:
            continue
        img, kps = detected[c["name"]]
        q = S.quotas(oracle, c["size"], c["nfeatures"])
        for l in range(8):
            r = np.sort(kps["response"][kps["octave"] == l])[::-1]
            if len(r) > q[l]:
                assert (r[q[l] - 1:] == r[q[l] - 1]).all(), (c["name"], l)
                seen += 1
    assert seen >= 8


@pytest.mark.parametrize("case", S.ORB_CASES, ids=lambda c: c["name"])
def test_in_capacity_cases_stay_inside_every_device_capacity(oracle, case):
    img = S.make(case)
    for num in NUMS:
        bits, cnt = S.device_capacity_bits(oracle, img, case["nfeatures"], num)
        assert bits == 0 and cnt["unknown"] == 0, (num, bits, cnt)


@pytest.mark.parametrize("case", S.OVERFLOW_CASES, ids=lambda c: c["name"])
def test_overflow_cases_cross_the_limit_they_are_meant_to_cross(oracle, case):
    bits, cnt = S.device_capacity_bits(oracle, S.make(case), case["nfeatures"], case["anms_num"], case["kp_capacity"])
    print(case["name"], bits, cnt)
    assert bits == case["bits"] and cnt["unknown"] == case["may"], (bits, cnt)


def test_matcher_frame_has_duplicate_descriptor_rows(oracle):
    M = S.MATCHER_TILED
    k, d = oracle.feature_detection(S.make(S.CASE[M["case"]]), 3000, M["anms_num"])
    assert (len(d), S.duplicate_rows(d)) == (M["rows"], M["oracle"]) and M["floor"] == M["oracle"] // 2 > 0


def test_keypoint_dtype_is_the_oracles(oracle):
    assert S.KEYPOINT_DTYPE == oracle.KEYPOINT_DTYPE


# ------------------------------------------------------------------------------------------------ (b) oracle vs numpy restatements
def _anms_from_radii(kps, num):
    if len(kps) < num:
        return kps
    order, rad = S.anms_radii(kps)
    return kps[order][rad >= np.sort(rad)[::-1][num - 1]]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in ("x", "y", "response", "octave", "angle"))


def test_vectorised_anms_equals_the_line_by_line_one(oracle, detected):
    """S.anms_radii (used below on the 3000-keypoint cases) against the line-by-line restatement, on the small cases and on tied user keypoints"""
    sets = [detected[n][1] for n in ("tile20_odd", "mirror_odd", "blobs_odd")] + [S.tied_keypoints(600, 4), S.tied_keypoints(500, 1)]
    for kps in sets:
        for num in (50, 200, len(kps)):
            assert _same(_anms_from_radii(kps, num), N.anms_numpy(kps, num))


@pytest.mark.parametrize("case", S.ORB_CASES, ids=lambda c: c["name"])
def test_anms_with_ties_matches_numpy(oracle, detected, case):
    kps = detected[case["name"]][1]
    nums = [n for n in NUMS if n <= len(kps)] + [n for n, _ in S.anms_tie_nums(kps)]
    for num in nums:
        assert _same(oracle.anms(kps, num), _anms_from_radii(kps, num)), num
    for num, want in S.anms_tie_nums(kps):
        assert len(oracle.anms(kps, num)) == want >= num


def test_anms_num_inside_a_radius_tie_keeps_the_whole_group(oracle, detected):
    kps = detected["tile20"][1]
    hits = [(num, n) for num, n in S.anms_tie_nums(kps) if n > num]
    assert len(hits) >= 2, hits
    user = S.tied_keypoints(2000, 4)
    assert sum(n > num for num, n in S.anms_tie_nums(user)) >= 2


def test_anms_all_equal_responses_returns_everything_in_input_order(oracle, detected):
    """3000 keypoints with one response: nobody is 1.11 x stronger than anybody, every radius is DBL_MAX, all are kept -- in the stable order, i.e. input order"""
    kps = detected["mirror"][1][:3000].copy()
    assert len(kps) == 3000
    kps["response"] = np.float32(0.0123)
    for num in (1, 500, 3000):
        got = oracle.anms(kps, num)
        assert _same(got, kps) and _same(got, N.anms_numpy(kps, num))
    neg = kps.copy(); neg["response"] = np.float32(-0.5)    # 1.11 x a negative response is SMALLER: equal responses now suppress each other, in input order
    assert _same(oracle.anms(neg, 500), _anms_from_radii(neg, 500))
    assert _same(oracle.anms(neg[:400], 100), N.anms_numpy(neg[:400], 100))


def _harris_map(img):
    """harris_numpy for every pixel at once (same integers, same float32 operations)"""
    I = img.astype(np.int64)
    Ix = np.zeros_like(I); Iy = np.zeros_like(I)
    Ix[1:-1, 1:-1] = (I[1:-1, 2:] - I[1:-1, :-2]) * 2 + (I[:-2, 2:] - I[:-2, :-2]) + (I[2:, 2:] - I[2:, :-2])
    Iy[1:-1, 1:-1] = (I[2:, 1:-1] - I[:-2, 1:-1]) * 2 + (I[2:, :-2] - I[:-2, :-2]) + (I[2:, 2:] - I[:-2, 2:])

    def box(A):
        c = np.pad(A, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
        out = np.zeros_like(A)
        out[3:-3, 3:-3] = c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]
        return out
    f = np.float32
    a, b, c = box(Ix * Ix).astype(f), box(Iy * Iy).astype(f), box(Ix * Iy).astype(f)
    scale = f(1.0) / (f(4) * f(7) * f(255)); s4 = scale * scale * scale * scale
    return (a * b - c * c - f(0.04) * (a + b) * (a + b)) * s4


@pytest.mark.parametrize("name", ["tile20", "tile97", "mirror", "checker8", "binary3", "tile20_odd", "mirror_odd"])
def test_selection_at_the_cut_matches_numpy(oracle, detected, name):
    """the detector's selection of every level restated: FAST corners inside the border, retainBest(2 q) on the score, Harris, retainBest(q) on
    the response, both with ties at the cut kept; the tied Harris responses are tied in the numpy restatement too (the ties are real)"""
    case = S.CASE[name]
    img, kps = detected[name]
    L = oracle.orb_layout(img.shape[1], img.shape[0], case["nfeatures"])
    lv = oracle.build_pyramid(img, 8, case["nfeatures"])
    ties_checked = over = 0
    for l in range(8):
        w, h, q = L["w"][l], L["h"][l], L["nfeat"][l]
        c = oracle.fast9_16(lv[l], 20, True)
        c = c[(c["x"] >= 31) & (c["x"] < w - 31) & (c["y"] >= 31) & (c["y"] < h - 31)]
        keep = N.retain_best_numpy(c["response"], 2 * q)
        assert np.array_equal(oracle.retain_best(c, 2 * q)["x"], c["x"][keep]) and len(oracle.retain_best(c, 2 * q)) == len(keep)
        c = c[keep]
        H = _harris_map(lv[l])
        xs, ys = c["x"].astype(int), c["y"].astype(int)
        resp = H[ys, xs]
        sample = np.linspace(0, len(c) - 1, min(len(c), 40)).astype(int) if len(c) else []
        for i in sample:
            assert oracle.harris_response(lv[l], xs[i], ys[i]) == resp[i] == N.harris_numpy(lv[l], xs[i], ys[i])
        sel = N.retain_best_numpy(resp, q)
        got = kps[kps["octave"] == l]
        s = np.float32(L["scale"][l])
        assert len(got) == len(sel), (l, len(got), len(sel))
        assert np.array_equal(got["x"], c["x"][sel] * s) and np.array_equal(got["y"], c["y"][sel] * s) and np.array_equal(got["response"], resp[sel])
        over += len(sel) > q
        # pairs the oracle reports as tied: the numpy Harris of both is the same float too
        u, inv, cnt = np.unique(got["response"], return_inverse=True, return_counts=True)
        r2 = resp[sel]
        for g in np.nonzero(cnt > 1)[0]:
            idx = np.nonzero(inv == g)[0]
            assert (r2[idx] == r2[idx[0]]).all()
            ties_checked += len(idx) - 1
    assert ties_checked >= case["floor"]["dup"] and (over >= 1 or "over" not in case["floor"])


@pytest.mark.parametrize("name", ["tile32", "checker8", "binary3", "blobs", "steps"])
def test_fast_matches_definition_on_structured_images(oracle, detected, name):
    img = detected[name][0][:200, :420]
    corner, score = N.fast_numpy(img, 20)
    kps = oracle.fast9_16(img, 20, nonmax=False)
    got = np.zeros_like(corner)
    got[kps["y"].astype(int) - 3, kps["x"].astype(int) - 3] = True
    assert np.array_equal(got, corner)
    ys, xs = np.nonzero(corner)
    for y, x in list(zip(ys, xs))[::max(1, len(ys) // 200)]:
        assert oracle.fast_corner_score(img, x + 3, y + 3, 20) == score[y, x]
    # 3 x 3 non-maximum suppression is STRICT: of two equal neighbouring scores neither survives (a flat blob has no keypoint)
    sc = np.zeros(img.shape, np.int64); sc[3:-3, 3:-3] = np.where(corner, score, 0)
    nb = np.stack([np.roll(np.roll(sc, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]).max(0)
    keep = (sc > nb) & (sc > 0)
    keep[:3] = keep[-3:] = False; keep[:, :3] = keep[:, -3:] = False
    kn = oracle.fast9_16(img, 20, nonmax=True)
    got = np.zeros_like(keep); got[kn["y"].astype(int), kn["x"].astype(int)] = True
    assert np.array_equal(got, keep)
    if name == "steps":
        assert not corner.any()


def test_rbrief_on_flat_and_symmetric_patches(oracle):
    pat = N.pattern_from_header()
    for n_img, (img, kps) in enumerate(S.flat_and_symmetric_keypoints()):
        out_k, desc = oracle.orb_compute(img, kps)
        assert len(out_k) > 0
        lv = oracle.build_pyramid(img, 8, 500)
        L = oracle.orb_layout(img.shape[1], img.shape[0], 500)
        blurs = [np.pad(oracle.gaussian_blur7(lv[l]), 32, mode="reflect") for l in range(4)]   # (a pattern point can leave a coarse level by a few pixels)
        for kp, d in zip(out_k, desc):
            l = int(kp["octave"])
            s = np.float32(1.0) / np.float32(L["scale"][l])
            cx = int(np.rint(np.float32(kp["x"]) * s)); cy = int(np.rint(np.float32(kp["y"]) * s))
            if min(cx, cy, lv[l].shape[1] - 1 - cx, lv[l].shape[0] - 1 - cy) < 19:
                continue   # within reach of the level border: the oracle reads copyMakeBorder's UNBLURRED border there (covered by the near-border tests)
            assert np.array_equal(d, N.rbrief_numpy(blurs[l], cx + 32, cy + 32, kp["angle"], pat)), (n_img, kp)
        if n_img == 0:
            assert not desc.any()          # flat: every comparison is a < a


def test_ic_angle_on_zero_moments(oracle):
    """flat patches and patches symmetric about the keypoint have m01 == m10 == 0 -> fastAtan2(0, 0) == 0 exactly; symmetric about one axis -> a multiple of 90"""
    flat = np.full((80, 80), 200, np.uint8)
    assert oracle.ic_angle(flat, 40, 40) == 0.0 == oracle.fast_atan2(0.0, 0.0)
    blobs = S.blob_lattice(120, 160, pitch=30, half=1)
    assert N.ic_moments(blobs, 70, 70) == (0, 0) and oracle.ic_angle(blobs, 70, 70) == 0.0
    chk = S.checkerboard(120, 160, 15)      # odd squares: the centre pixel of a square (52, 52) is a centre of symmetry
    zero = 0
    for (x, y) in [(52, 52), (67, 52), (52, 67), (45, 45), (60, 52), (48, 47), (50, 61)]:
        m01, m10 = N.ic_moments(chk, x, y)
        assert oracle.ic_angle(chk, x, y) == oracle.fast_atan2(np.float32(m01), np.float32(m10))
        zero += (m01, m10) == (0, 0)
    assert zero >= 3
    steps = S.step_edges(80, 120)
    m01, m10 = N.ic_moments(steps, 60, 40)
    assert m01 == 0 and m10 != 0 and oracle.ic_angle(steps, 60, 40) in (0.0, 180.0)


def test_detected_zero_angles_are_zero_moments(oracle, detected):
    img, kps = detected["checker8"]
    L = oracle.orb_layout(img.shape[1], img.shape[0], 3000)
    lv = oracle.build_pyramid(img, 8, 3000)
    z = kps[kps["angle"] == 0][:10]
    assert len(z) >= 5
    for kp in z:
        l = int(kp["octave"]); s = np.float32(1.0) / np.float32(L["scale"][l])
        x = int(np.rint(np.float32(kp["x"]) * s)); y = int(np.rint(np.float32(kp["y"]) * s))
        m01, m10 = N.ic_moments(lv[l], x, y)
        assert m01 == 0 and m10 >= 0


# ------------------------------------------------------------------------------------------------ (c) SGBM known answers
@pytest.mark.parametrize("size", S.KNOWN_ANSWER_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("pair", S.SGBM_CLEAN, ids=lambda c: "p%d_s%d" % (c["period"], c["shift"]))
def test_sgbm_periodic_pair_known_answer(oracle, pair, size):
    """every pixel with x >= 96 is valid and equals shift mod period -- the FIRST of the tied minima d, d + p, d + 2p --, the columns left of 96 are -1"""
    w, h = size
    L, R = S.periodic_pair(w=w, h=h, **pair)
    s, p = pair["shift"], pair["period"]
    assert s < S.NUM_DISP and np.array_equal(L[:, s:], R[:, :w - s]) and (s + p >= S.NUM_DISP or np.array_equal(L[:, s + p:], R[:, :w - s - p]))
    f = oracle.disparity_map(L, R)
    assert (f[:, :96] == -1).all()
    assert (f[:, 96:] == float(s % p)).all(), np.unique(f[:, 96:], return_counts=True)
    d16, raw = oracle.sgbm_compute(L, R, return_raw=True)
    assert ((raw[:, 96:] + 8) >> 4 == s % p).all()       # the winner before the median / speckle filters, whole pixels


def test_sgbm_residues_cover_zero_small_and_large():
    for p in (24, 32, 48, 64):
        r = sorted(c["shift"] % p for c in S.SGBM_CLEAN if c["period"] == p)
        assert r[0] == 0 and 0 < r[1] <= p // 2 and r[2] > p // 2, (p, r)
        assert all(c["shift"] < 96 for c in S.SGBM_CLEAN)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_sgbm_periodic_winner_for_other_seeds(oracle, seed):
    """the whole-pixel winner is shift mod period for any texture (the 1/16 refinement may move a pixel or two per image by one step, see periodic_pair)"""
    for p, s in ((24, 67), (32, 5), (48, 40), (64, 70)):
        L, R = S.periodic_pair(p, s, seed=seed)
        d16 = oracle.sgbm_compute(L, R)
        assert (d16[:, 96:] >= 0).all() and ((d16[:, 96:] + 8) >> 4 == s % p).all()
        assert (d16[:, 96:] != 16 * (s % p)).sum() <= 8


def test_sgbm_kitti_sized_periodic_pair_known_answer(oracle):
    k = S.KITTI_PERIODIC
    for s in (5, 37, 64):
        L, R = S.periodic_pair(shift=s, **k)
        f = oracle.disparity_map(L, R)
        assert f.shape == (376, 1241) and (f[:, :96] == -1).all() and (f[:, 96:] == float(s % k["period"])).all()


@pytest.mark.parametrize("pair", S.SGBM_NOISY, ids=lambda c: "p%d_s%d_n%d" % (c["period"], c["shift"], c["noise"]))
def test_sgbm_noisy_periodic_pair_splits_between_tied_winners(oracle, pair):
    L, R = S.periodic_pair(pair["period"], pair["shift"], pair["noise"])
    d16 = oracle.sgbm_compute(L, R)
    share = S.sgbm_winner_shares(d16)
    print(pair["period"], pair["shift"], pair["noise"], {k: round(v, 4) for k, v in share.items() if v > 0.005})
    assert len(pair["winners"]) >= 2 and len({d % pair["period"] for d in pair["winners"]}) == 1
    for d, fig in pair["winners"].items():
        assert share.get(d, 0.0) >= fig["floor"], (d, share.get(d, 0.0), fig)
        assert abs(fig["floor"] - fig["oracle"] / 2) < 1e-4 and abs(share[d] - fig["oracle"]) < 5e-5    # the recorded share is current, the floor is half of it
