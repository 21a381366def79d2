"""K1's wave-typed instances keep their register budgets.  k_autocorr_wt<3, false, 8> (the headline's
K1 with K2 as its tail) and k_autocorr_wt<4, false, 12> (configs[3]'s) run one 512-thread workgroup per
CU: two waves per SIMD, so at most 256 VGPRs, no vector spills and no scratch.  The LPC-12 tail spills
SGPRs into VGPR lanes; that count must not grow past what it was before the even lag group took its
second operand from registers (265 for <4, false, 12>, 273 for <3, false, 12>).  Runs without a GPU:
hipcc cross-compiles k1_autocorr.hip with -Rpass-analysis=kernel-resource-usage, as
tools/kernel_resources.py does."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flake_amd import build as fb  # noqa: E402

# instance -> largest SGPR spill count allowed
BUDGET = {
    "k_autocorr_wt<3, false, 8>": 8,
    "k_autocorr_wt<3, false, 12>": 273,
    "k_autocorr_wt<4, false, 12>": 265,
}

pytestmark = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def resources():
    cmd = [fb.HIPCC, *[x for x in fb.HIP_FLAGS if x != "-shared"], "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(fb.PKG, "csrc"), "--cuda-device-only", "-c",
           os.path.join(fb.PKG, "csrc", "k1_autocorr.hip"), "-o", os.devnull,
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
    out = {}
    for mangled, res in kernels.items():
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout
        for inst in BUDGET:
            if inst in name:
                out[inst] = res
    missing = set(BUDGET) - set(out)
    assert not missing, f"{sorted(missing)} not found among {len(kernels)} kernels:\n{err[-2000:]}"
    return out


@pytest.mark.parametrize("inst", sorted(BUDGET))
def test_one_workgroup_per_cu_without_vector_spills(resources, inst):
    r = resources[inst]
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, r
    assert r["Occupancy [waves/SIMD]"] >= 2, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r


@pytest.mark.parametrize("inst", sorted(BUDGET))
def test_sgpr_spills_within_budget(resources, inst):
    r = resources[inst]
    assert r["SGPRs Spill"] <= BUDGET[inst], r
