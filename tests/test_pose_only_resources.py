"""Occupancy of pose_only_wave_kernel's instantiations, read from the code-object notes of libvslam_hip.so (no GPU needed).

The narrow form exists to put several windows on a CU at the register count of the 12-wave form.  A SIMD lane has 512 registers, allocated in
steps of 8, at most 8 waves per SIMD; a CU has 4 SIMDs and 160 KB of LDS.  VSLAM_MAX_KF = 12 waves at three per SIMD (168 registers) fill a CU; the narrow
form is 4 waves at two per SIMD (up to 256 registers, so that nothing spills): two workgroups per CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "stereo-visual-slam_amd", "libvslam_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KF_MAX = 12
NARROW = {4: 2}   # waves per window of the narrow form: workgroups per CU it is built for


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{W: notes of pose_only_wave_kernel<W>}"""
    if not (os.path.exists(SO) and os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("libvslam_hip.so or the LLVM tools are missing")
    d = str(tmp_path_factory.mktemp("codeobj"))
    so = os.path.join(d, "lib.so")
    shutil.copy(SO, so)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f:
            continue
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(d, f)], check=True, capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
            name = re.search(r"\.name:\s+\S*pose_only_wave_kernelILi(\d+)E", blk)
            if not name:
                continue
            g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
            out[int(name.group(1))] = dict(vgpr=g("vgpr_count"), lds=g("group_segment_fixed_size"), wg=g("max_flat_workgroup_size"))
    return out


def _workgroups_per_cu(k, W):
    alloc = (k["vgpr"] + 7) // 8 * 8
    waves_per_simd = min(8, 512 // alloc)
    return min(4 * waves_per_simd // W, (160 * 1024) // k["lds"], 32 // W)


def test_two_forms_are_built(forms):
    assert KF_MAX in forms and len(forms) == 2, sorted(forms)
    for W, k in forms.items():
        assert k["wg"] == 64 * W, (W, k)


def test_one_keyframe_per_wave_keeps_its_registers(forms):
    k = forms[KF_MAX]
    assert k["vgpr"] <= 168, k
    assert _workgroups_per_cu(k, KF_MAX) == 1


def test_narrow_form_shares_a_cu(forms):
    (W,) = [w for w in forms if w != KF_MAX]
    k = forms[W]
    assert W in NARROW, (W, k)
    assert _workgroups_per_cu(k, W) >= NARROW[W], (W, k, _workgroups_per_cu(k, W))
