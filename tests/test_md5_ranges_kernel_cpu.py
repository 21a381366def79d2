"""k_md5_ranges (k6_md5.hip), K6's update over ranges that the device names: every instance is there and compiles for
gfx950 without scratch, without spills and without AGPRs, as tests/test_md5_kernel_cpu.py asks of the kernels it
knows.  Runs without a GPU.  The register and LDS figures are printed (pytest -s) and recorded in DESIGN.md."""
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
    found, err = _resources(os.path.join(fb.PKG, "csrc", "k6_md5.hip"))
    named = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip(): v for k, v in found.items()}
    assert named, err[-2000:]
    return {k: v for k, v in named.items() if "k_md5_ranges" in k}


def test_every_instance_is_there(kernels):
    assert len(kernels) == len(INSTANCES), sorted(kernels)
    for inst in INSTANCES:
        assert sum(("k_md5_ranges" + inst) in name for name in kernels) == 1, (inst, sorted(kernels))


def test_no_scratch_no_spills_no_agprs(kernels):
    assert len(kernels) == len(INSTANCES), sorted(kernels)
    for name, res in sorted(kernels.items()):
        print(f"{re.search(r'k_md5_ranges<[^>]*>', name).group(0)}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, "
              f"{res['LDS Size [bytes/block]']} bytes of LDS")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)
        assert res["LDS Size [bytes/block]"] == 4096, (name, res)       # the tails of 64 lanes, nothing else
