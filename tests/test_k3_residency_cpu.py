"""K3's lean instance k_encode_pow2<16, 256, 0> -- the headline's encode kernel -- keeps SEVEN workgroups
per CU: at most 72 VGPRs, no scratch, at most 96 SGPRs (.sgpr_count 82-96 still admits seven 256-thread
blocks), and an LDS layout at the headline's parameters that fits seven times into 160 KiB.  A change that
quietly costs a workgroup fails here.  Runs without a GPU: hipcc cross-compiles k3_encode.hip with
-Rpass-analysis=kernel-resource-usage (as tools/kernel_resources.py does) and a host program prints
fast_lds_layout() for the headline launch."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flake_amd import build as fb  # noqa: E402

KERNEL = "k_encode_pow2<16, 256, 0>"
WG_PER_CU = 7                      # 256-thread workgroups: one wave per SIMD each
LDS_PER_CU = 160 * 1024

pytestmark = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")


def _cflags():
    return [*[x for x in fb.HIP_FLAGS if x != "-shared"], "-I", os.path.join(ROOT, "include"),
            "-I", os.path.join(fb.PKG, "csrc")]


def _resources(src):
    cmd = [fb.HIPCC, *_cflags(), "--cuda-device-only", "-c", src, "-o", os.devnull,
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
    return kernels, err


@pytest.fixture(scope="module")
def lean():
    kernels, err = _resources(os.path.join(fb.PKG, "csrc", "k3_encode.hip"))
    names = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout: k for k in kernels}
    hit = [k for d, k in names.items() if KERNEL in d]
    assert len(hit) == 1, f"{KERNEL} not found among {len(kernels)} kernels:\n{err[-2000:]}"
    return kernels[hit[0]]


def test_lean_encode_registers_admit_seven_waves_per_simd(lean):
    assert lean["VGPRs"] <= 72, lean
    assert lean.get("AGPRs", 0) == 0, lean
    assert lean["Occupancy [waves/SIMD]"] >= WG_PER_CU, lean


def test_lean_encode_has_no_scratch(lean):
    assert lean["ScratchSize [bytes/lane]"] == 0, lean
    assert lean["VGPRs Spill"] == 0 and lean["SGPRs Spill"] == 0, lean


def test_lean_encode_sgprs_admit_seven_workgroups(lean):
    assert lean["TotalSGPRs"] <= 96, lean


def test_headline_lds_fits_seven_workgroups(tmp_path):
    import flake_amd
    p = flake_amd.level_params(5, order_method=flake_amd.OM_MAX)        # bench.py's configs[1]
    assert p.block_size == 16 * 256
    src = tmp_path / "lds.hip"
    src.write_text(
        '#include <cstdio>\n#include "k3_common.h"\nusing namespace fhip;\n'
        "int main() {\n"
        "    size_t off[11];\n"
        f"    const size_t b = fast_lds_layout({p.block_size}, SmpImg<16, 256>::SIZE, off,\n"
        f"                                     fast_wide_window(0, {p.bits_per_sample}),\n"
        f"                                     fast_heap_nodes(0, {p.max_partition_order}), true);\n"
        '    std::printf("%zu\\n", b);\n'
        "    return 0;\n}\n")
    exe = tmp_path / "lds"
    subprocess.run([fb.HIPCC, *[x for x in _cflags() if x not in ("-fPIC", "-fvisibility=hidden")],
                    "--cuda-host-only", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=600)
    lds = int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)
    assert lds % 16 == 0
    assert LDS_PER_CU // lds >= WG_PER_CU, lds
