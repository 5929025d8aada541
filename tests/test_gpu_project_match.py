"""GPU: vslam_project_match_dev bit for bit against the yardstick (project_match_ref.py) on the shared cases (project_match_cases.py; the CPU guard
test_project_match_ref.py keeps every case a margin away from the bounds of the f64 steps, so the remaining steps are integers), the invalid
inputs, the refused arguments, determinism, and an item alone against the item in a batch."""
import ctypes as C

import numpy as np
import pytest

import project_match_cases as PC
import project_match_ref as R

pytestmark = pytest.mark.gpu

CASES = PC.all_cases()
INVALID = PC.invalid_cases()
KEYS = ("status", "match", "dist", "n_cand")


@pytest.fixture(scope="module")
def contexts(pkg, vo):
    small = pkg.VO(device=0, max_batch=1, img_w=64, img_h=64)
    yield {(1241, 376): vo, (64, 64): small}
    small.close()


@pytest.fixture(scope="module")
def answers():
    return {c["name"]: PC.reference(c, out=PC.sentinel_out(len(c["lm_desc_row"]))) for c in CASES}


def run(pkg, contexts, c, fill=PC.FILL, **override):
    kps = np.zeros(c["kps_xy"].shape[:2], pkg.KEYPOINT_DTYPE)
    kps["x"] = c["kps_xy"][..., 0]; kps["y"] = c["kps_xy"][..., 1]
    return contexts[(c["w"], c["h"])].project_match(c["lm_off"], c["item_img"], c["item_T"], c["lm_xyz"], c["lm_desc_row"], c["src_desc"], kps, c["desc"], c["n"],
                                                     K4=c["K4"], fill=fill, **dict(c["params"], **override))


def same(got, want, what):
    for key in KEYS:
        bad = np.flatnonzero(got[key] != want[key])
        assert bad.size == 0, "%s: %s differs at %d landmarks, first %d: device %d, yardstick %d (status %d / %d)" % (
            what, key, bad.size, bad[0], got[key][bad[0]], want[key][bad[0]], got["status"][bad[0]], want["status"][bad[0]])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_parity(pkg, contexts, answers, c):
    same(run(pkg, contexts, c), answers[c["name"]], c["name"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_parity_with_the_descriptors_staged_in_lds(pkg, contexts, answers, c):
    """the kernel's other form (set_tuning pm_stage = 1: the image's descriptors copied into LDS first): the same bytes"""
    ctx = contexts[(c["w"], c["h"])]
    ctx.set_tuning(pm_stage=1)
    try:
        same(run(pkg, contexts, c), answers[c["name"]], c["name"])
    finally:
        ctx.set_tuning(pm_stage=-1)


@pytest.mark.parametrize("c, bad", INVALID, ids=[c["name"] for c, _ in INVALID])
def test_invalid_inputs(pkg, contexts, c, bad):
    """INVALID for exactly the affected landmarks; what no item owns keeps the sentinel; everything else is the yardstick's answer"""
    want = PC.reference(c, out=PC.sentinel_out(len(c["lm_desc_row"])))
    assert np.flatnonzero(want["status"] == R.INVALID).tolist() == bad
    got = run(pkg, contexts, c)
    same(got, want, c["name"])
    assert (got["match"][bad] == -1).all() and (got["dist"][bad] == -1).all()


def test_same_call_twice_same_bytes(pkg, contexts):
    c = next(c for c in CASES if c["name"] == "random_8x700x900")
    a, b = run(pkg, contexts, c), run(pkg, contexts, c)
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_item_alone_equals_item_in_batch(pkg, contexts, answers):
    c = next(c for c in CASES if c["name"] == "random_8x700x900")
    whole = answers[c["name"]]
    for m in (0, 1, 5):
        lo, hi = int(c["lm_off"][m]), int(c["lm_off"][m + 1])
        alone = dict(c, lm_off=np.array([0, hi - lo], np.int32), item_img=c["item_img"][m:m + 1], item_T=c["item_T"][m:m + 1], lm_xyz=c["lm_xyz"][lo:hi],
                     lm_desc_row=c["lm_desc_row"][lo:hi])
        same(run(pkg, contexts, alone), {k: v[lo:hi] for k, v in whole.items()}, "item %d alone" % m)


def test_n_cand_is_optional(pkg, vo):
    import torch
    c = next(c for c in CASES if c["name"] == "kitti")
    dev = torch.device("cuda:0")
    kps = np.zeros(c["kps_xy"].shape[:2], pkg.KEYPOINT_DTYPE)
    kps["x"] = c["kps_xy"][..., 0]; kps["y"] = c["kps_xy"][..., 1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = dict(off=up(c["lm_off"]), img=up(c["item_img"]), T=up(c["item_T"]), xyz=up(c["lm_xyz"]), row=up(c["lm_desc_row"]), src=up(c["src_desc"]), kps=up(kps.view(np.uint8)),
             desc=up(c["desc"]), n=up(c["n"]))
    B, cap = kps.shape
    batch = pkg.ProjectMatchBatch(n_items=len(c["item_img"]), n_landmarks=len(c["lm_desc_row"]), B=B, kp_capacity=cap, n_src_rows=len(c["src_desc"]),
                                  d_lm_off=t["off"].data_ptr(), d_item_img=t["img"].data_ptr(), d_item_T=t["T"].data_ptr(), d_lm_xyz=t["xyz"].data_ptr(),
                                  d_lm_desc_row=t["row"].data_ptr(), d_src_desc=t["src"].data_ptr(), d_kps=t["kps"].data_ptr(), d_desc=t["desc"].data_ptr(),
                                  d_n=t["n"].data_ptr())
    torch.cuda.synchronize()
    out = vo.project_match_dev(batch, pkg.default_project_match_params(**c["params"]), n_cand=False)
    vo.sync()
    assert out["n_cand"] is None
    want = PC.reference(c)
    for key in ("status", "match", "dist"):
        assert np.array_equal(out[key].cpu().numpy(), want[key]), key


def test_refused_arguments(pkg, vo):
    import torch
    dev = torch.device("cuda:0")
    buf = torch.zeros(4096, dtype=torch.uint8, device=dev)
    p0 = buf.data_ptr()
    assert p0 % 16 == 0

    def batch(**kw):
        f = dict(n_items=1, n_landmarks=1, B=1, kp_capacity=8, n_src_rows=1, d_lm_off=p0, d_item_img=p0, d_item_T=p0, d_lm_xyz=p0, d_lm_desc_row=p0, d_src_desc=p0,
                 d_kps=p0, d_desc=p0, desc_stride_bytes=0, d_n=p0, d_match=p0, d_dist=p0, d_n_cand=None, d_status=p0)
        f.update(kw)
        b = pkg.ProjectMatchBatch(**f)
        b.struct_size = C.sizeof(pkg.ProjectMatchBatch)
        return b

    def refused(b, p=None, word=None):
        rc = vo.lib.vslam_project_match_dev(vo.h, C.byref(b), None if p is None else C.byref(p))
        assert rc == pkg.VSLAM_ERR_ARG, (rc, word)
        msg = vo.lib.vslam_last_error().decode()
        assert "vslam_project_match_dev" in msg and (word is None or word in msg), msg

    for field in ("d_lm_off", "d_item_img", "d_item_T", "d_lm_xyz", "d_lm_desc_row", "d_src_desc", "d_kps", "d_desc", "d_n", "d_match", "d_dist", "d_status"):
        refused(batch(**{field: None}), word="null")
    refused(batch(n_items=0), word="n_items"); refused(batch(B=0), word="B"); refused(batch(n_landmarks=-1)); refused(batch(n_src_rows=-1))
    refused(batch(kp_capacity=0), word="kp_capacity"); refused(batch(kp_capacity=pkg.PROJECT_MATCH_MAX_KP + 1), word="kp_capacity")
    refused(batch(d_src_desc=p0 + 8), word="aligned"); refused(batch(d_desc=p0 + 4), word="aligned")
    refused(batch(desc_stride_bytes=8 * 32 + 8), word="desc_stride_bytes"); refused(batch(desc_stride_bytes=7 * 32), word="desc_stride_bytes")
    b = batch(); b.struct_size -= 8
    refused(b, word="struct_size")
    p = pkg.default_project_match_params(); p.struct_size += 4
    refused(batch(), p, word="struct_size")
    for kw, word in ((dict(radius_px=0.0), "radius_px"), (dict(radius_px=-1.0), "radius_px"), (dict(radius_px=float("inf")), "radius_px"), (dict(radius_px=float("nan")), "radius_px"),
                     (dict(tau=-1), "tau"), (dict(tau=256), "tau"), (dict(ratio_pct=-1), "ratio_pct"), (dict(ratio_pct=101), "ratio_pct"), (dict(z_min=float("nan")), "gate")):
        refused(batch(), pkg.default_project_match_params(**kw), word=word)
    k4 = (C.c_double * 4)(0.0, 100.0, 1.0, 1.0)
    refused(batch(K4=C.cast(k4, C.POINTER(C.c_double))), word="camera")
    rc = vo.lib.vslam_project_match_dev(None, C.byref(batch()), None)
    assert rc == pkg.VSLAM_ERR_ARG
    # nothing was launched: the buffer every pointer named is still zero
    vo.sync()
    assert int(buf.sum()) == 0
