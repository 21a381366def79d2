"""K6 (k6_md5.hip) keeps its hash in registers: every k_md5_streams instance compiles for gfx950 without scratch
and without vector or scalar spills -- a register array that the compiler could only index through memory would show
up here.  Runs without a GPU: hipcc cross-compiles the file with -Rpass-analysis=kernel-resource-usage, as
tests/test_k3_residency_cpu.py does.  The VGPR counts are printed (pytest -s) and recorded in DESIGN.md; they are not
bounded here."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flake_amd import build as fb  # noqa: E402
from test_k3_residency_cpu import _resources  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

INSTANCES = ("<short, 1>", "<short, 2>", "<int, 1>", "<int, 2>", "<int, 3>", "<int, 4>")


@pytest.fixture(scope="module")
def kernels():
    src = os.path.join(fb.PKG, "csrc", "k6_md5.hip")
    assert "csrc/k6_md5.hip" in fb.HIP_SRCS
    found, err = _resources(src)
    named = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip(): v for k, v in found.items()}
    assert named, err[-2000:]
    return named


def test_every_instance_is_there(kernels):
    for inst in INSTANCES:
        assert sum(("k_md5_streams" + inst) in name for name in kernels) == 1, (inst, sorted(kernels))
    for other in ("k_md5_init", "k_md5_scan", "k_md5_final"):
        assert any(other in name for name in kernels), other


def test_no_scratch_and_no_spills(kernels):
    for name, res in sorted(kernels.items()):
        if "k_md5" not in name:
            continue
        print(f"{re.search(r'k_md5_[a-z]+(<[^>]*>)?', name).group(0)}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, "
              f"{res['LDS Size [bytes/block]']} bytes of LDS")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)
