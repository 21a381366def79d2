"""int16 PCM (fhip_set_pcm_format / flake_amd_encode_frames_s16) without a GPU.

The two entries exist and refuse a null handle.  K0's int16 instances keep the register budgets of their
int32 twins: hipcc cross-compiles k0_prepare.hip with -Rpass-analysis=kernel-resource-usage (as
tests/test_k1_residency_cpu.py does for K1) and every int16 instance checked -- the stereo instances of the
geometries FHIP_STEREO_GEOM picks for n = 1152, 4096 and 8192, and k_prepare_multi_reg_s16<1, 1> / <8, 1> --
must have no scratch, no vector spills, and VGPRs and waves per SIMD no worse than the int32 instance of the
same geometry IN THE SAME COMPILE.  The twin is code the int16 change does not touch, so it is the yardstick
rather than a number written down here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402

# int16 instance -> its int32 twin (demangled spellings)
TWINS = {
    "k_prepare_stereo_s16<5, 1>": "k_prepare_stereo<5, 1, true>",        # n = 1152
    "k_prepare_stereo_s16<4, 4>": "k_prepare_stereo<4, 4, true>",        # n = 4096
    "k_prepare_stereo_s16<8, 4>": "k_prepare_stereo<8, 4, true>",        # n = 8192
    "k_prepare_multi_reg_s16<1, 1>": "k_prepare_multi_reg<1, 1>",
    "k_prepare_multi_reg_s16<8, 1>": "k_prepare_multi_reg<8, 1>",
}


def test_entries_are_exported_and_refuse_a_null_handle():
    lib = flake_amd.load_library()
    assert "fhip_set_pcm_format" in flake_amd.ABI_SYMBOLS
    assert lib.fhip_set_pcm_format(None, flake_amd.PCM_S16) == flake_amd.E_INVALID
    assert lib.fhip_set_pcm_format(None, flake_amd.PCM_S32) == flake_amd.E_INVALID
    host = flake_amd.load_host_library()
    buf = (C.c_int16 * 64)()
    out = (C.c_ubyte * 64)()
    assert host.flake_amd_encode_frames_s16(None, buf, 1, 16, 0, out, 64, None) == -1


def test_header_declares_the_format():
    text = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    assert re.search(r"enum\s*\{\s*FHIP_PCM_S32\s*=\s*0\s*,\s*FHIP_PCM_S16\s*=\s*1\s*\}", text)
    assert (flake_amd.PCM_S32, flake_amd.PCM_S16) == (0, 1)
    assert "flake_amd_encode_frames_s16" in open(os.path.join(ROOT, "include", "flake_amd.h")).read()


@pytest.fixture(scope="module")
def resources():
    cmd = [fb.HIPCC, *[x for x in fb.HIP_FLAGS if x != "-shared"], "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(fb.PKG, "csrc"), "--cuda-device-only", "-c",
           os.path.join(fb.PKG, "csrc", "k0_prepare.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=1800).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([A-Za-z][^:]*?): +(-?\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    wanted = set(TWINS) | set(TWINS.values())
    out = {}
    for mangled, res in kernels.items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout
        for inst in wanted:
            if inst + "(" in name:
                out[inst] = res
    missing = wanted - set(out)
    assert not missing, f"{sorted(missing)} not found among {len(kernels)} kernels:\n{err[-2000:]}"
    return out


@pytest.mark.parametrize("inst", sorted(TWINS))
def test_int16_instance_is_no_heavier_than_its_int32_twin(resources, inst):
    r, t = resources[inst], resources[TWINS[inst]]
    print(inst, r, "twin", t)
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= t["VGPRs"] + t.get("AGPRs", 0), (r, t)
    assert r["Occupancy [waves/SIMD]"] >= t["Occupancy [waves/SIMD]"], (r, t)
