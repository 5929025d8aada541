"""CPU: the caller-set StereoSGBM surface -- vslam_sgbm_params, its defaults and vslam_sgbm_params_check's domain (host arithmetic, no GPU) --
and the oracle guards of tests/test_gpu_sgbm_params.py: every (pair, set) of the GPU tests gives a map that differs from the reference set's, so
a library that ignored the set could not pass them."""
import os
import re

import numpy as np
import pytest

import sgbm_param_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct vslam_sgbm_params\s*\{[^}]*\}\s*vslam_sgbm_params;", hdr)
    for name in ("vslam_default_sgbm_params", "vslam_sgbm_params_check", "vslam_disparity_map_ex", "vslam_disparity_map_ex_dev"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    body = re.search(r"typedef struct vslam_sgbm_params\s*\{([^}]*)\}", hdr).group(1)
    fields = re.findall(r"\b([A-Za-z_0-9]+)\s*[,;]", body)
    assert fields == ["num_disparities", "block_size", "P1", "P2", "disp12_max_diff", "pre_filter_cap", "uniqueness_ratio", "speckle_window_size",
                      "speckle_range", "struct_size"]
    assert "#define VSLAM_ABI_VERSION 5" in hdr


def test_default_sgbm_params(pkg):
    import ctypes as C
    p = pkg.default_sgbm_params()
    assert p.as_tuple() == (96, 9, 648, 2592, 1, 63, 10, 100, 32)
    assert p.struct_size == C.sizeof(pkg.SgbmParams) == 40
    assert pkg.default_sgbm_params(num_disparities=64).as_tuple()[:2] == (64, 9)


def test_check_accepts_the_domain(pkg):
    assert pkg.sgbm_params_check(pkg.default_sgbm_params(), 1241, 376)
    assert pkg.sgbm_params_check(None, 1241, 376)   # NULL = the reference's set
    assert pkg.sgbm_params_check(cases.BOUNDARY, 260, 50)   # block 9, cap 63, P2 = 21845 - 15309 = 6536
    assert pkg.sgbm_params_check(cases.DB_SETS["d96_b11_cap31"], 300, 60)
    for name, s in cases.SETS.items():
        assert pkg.sgbm_params_check(s, 480, 40), name
    # the smallest admissible images
    assert pkg.sgbm_params_check(dict(num_disparities=16, block_size=1, P1=8, P2=32), 17, 2)
    assert pkg.sgbm_params_check(dict(), 101, 10) and pkg.sgbm_params_check(dict(), 4096, 10)
    assert pkg.sgbm_params_check(dict(speckle_window_size=0, speckle_range=0, disp12_max_diff=0, uniqueness_ratio=0, pre_filter_cap=1), 300, 60)


@pytest.mark.parametrize("name,s,w,h", cases.REFUSED, ids=[c[0] for c in cases.REFUSED])
def test_check_refuses(pkg, name, s, w, h):
    with pytest.raises(pkg.VslamError) as e:
        pkg.sgbm_params_check(s, w, h)
    assert "(-1)" in str(e.value)   # VSLAM_ERR_ARG
    field = {"D0": "num_disparities", "D24": "num_disparities", "D272": "num_disparities", "block_even": "block_size", "P1_0": "P1", "P1_eq_P2": "P2",
             "P1_gt_P2": "P2", "cap0": "pre_filter_cap", "cap64": "pre_filter_cap", "uniq_neg": "uniqueness_ratio", "uniq101": "uniqueness_ratio",
             "disp12_neg": "disp12_max_diff", "speckle_range_neg": "speckle_range", "too_narrow": "num_disparities", "too_narrow_d64_b7": "num_disparities",
             "too_low": "block_size", "too_wide": "width", "struct_size": "struct_size"}[name]
    assert field in str(e.value), str(e.value)


def test_check_beyond_the_range_rule_is_a_decision(pkg):
    """a set beyond 3 * (Cmax + P2) <= 65535 is refused or accepted; the GPU test holds an accepted one to the oracle"""
    for name, s in cases.BEYOND.items():
        try:
            assert pkg.sgbm_params_check(s, 260, 50) is True
        except pkg.VslamError as e:
            assert "16-bit" in str(e), name


def test_check_needs_no_context_and_speckle_window_negative(pkg):
    with pytest.raises(pkg.VslamError):
        pkg.sgbm_params_check(dict(speckle_window_size=-1), 300, 60)


@pytest.fixture(scope="module")
def default_maps(oracle):
    return {pn: oracle.sgbm_compute(L, R, return_raw=True) for pn, (L, R) in cases.pairs().items()}


@pytest.mark.parametrize("pn,sn", cases.host_cases(), ids=["%s-%s" % c for c in cases.host_cases()])
def test_oracle_guard_host_cases(oracle, default_maps, pn, sn):
    L, R = cases.pairs()[pn]
    disp, raw = oracle.sgbm_compute(L, R, return_raw=True, **cases.oracle_kwargs(cases.SETS[sn]))
    assert not np.array_equal(disp, default_maps[pn][0]), "this set's map equals the reference set's on this pair: the GPU case would prove nothing"


@pytest.mark.parametrize("sn", cases.DEVICE_B5_SETS)
def test_oracle_guard_device_b5_sets(oracle, synth, sn):
    pairs, _ = cases.batch(synth, 5, 300, 60, 320)
    kw = cases.oracle_kwargs(cases.SETS[sn])
    differs = [not np.array_equal(oracle.sgbm_compute(L, R, **kw), oracle.sgbm_compute(L, R)) for L, R in pairs]
    assert any(differs), "this set's maps equal the reference set's on all five pairs: the GPU case would prove nothing"


def test_oracle_guard_boundary(oracle):
    L, R = cases.saturated_pair()
    ref = oracle.sgbm_compute(L, R)
    assert not np.array_equal(oracle.sgbm_compute(L, R, **cases.oracle_kwargs(cases.BOUNDARY)), ref)
