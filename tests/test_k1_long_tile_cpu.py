"""K1's long-tile form (k_autocorr_wtl: 256 positions per hand-over on two LDS buffers) keeps the register
budget of one 512-thread workgroup per CU, and fhip_autocorr_tile tells which form a batch takes.

The long-form instances of the headline (<3, false, 8>), of the VBS levels (<3, false, 12>) and of configs[3]
(<4, false, 12>) run two waves per SIMD: at most 256 VGPRs, occupancy at least 2, no vector spills and no
scratch; their SGPR spills must not exceed those of the 128-form twin compiled beside them.  Runs without a
GPU: hipcc cross-compiles k1_autocorr.hip with -Rpass-analysis=kernel-resource-usage, as
tests/test_k1_residency_cpu.py does.

The order-12 instances used to spill 236 SGPRs (128 form) and 254 / 280 (long form), all of them in the K2 tail
(lpc_reg_one<12>); since the tail quantises its one row behind the recursion and searches the shift without
branches (lpc_reg.h), no instance of either form spills any."""
import os
import re
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402

INSTANCES = ["<3, false, 8>", "<3, false, 12>", "<4, false, 12>"]

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")


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
        for inst in INSTANCES:
            for form in ("k_autocorr_wtl", "k_autocorr_wt"):
                if form + inst in name:
                    out[form + inst] = res
    missing = {f + i for i in INSTANCES for f in ("k_autocorr_wtl", "k_autocorr_wt")} - set(out)
    assert not missing, f"{sorted(missing)} not found among {len(kernels)} kernels:\n{err[-2000:]}"
    return out


@needs_hipcc
@pytest.mark.parametrize("inst", INSTANCES)
def test_long_form_one_workgroup_per_cu_without_vector_spills(resources, inst):
    r = resources["k_autocorr_wtl" + inst]
    print(inst, r)
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, r
    assert r["Occupancy [waves/SIMD]"] >= 2, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r


@needs_hipcc
@pytest.mark.parametrize("inst", INSTANCES)
def test_long_form_sgpr_spills_not_above_the_128_form(resources, inst):
    long_form, twin = resources["k_autocorr_wtl" + inst], resources["k_autocorr_wt" + inst]
    print(inst, "long", long_form["SGPRs Spill"], "128 form", twin["SGPRs Spill"])
    assert long_form["SGPRs Spill"] <= twin["SGPRs Spill"], (long_form, twin)


def test_autocorr_tile_query(monkeypatch):
    monkeypatch.delenv("FHIP_WT_TILE", raising=False)
    monkeypatch.delenv("FHIP_AC_KERNEL", raising=False)
    tile = flake_amd.load_library().fhip_autocorr_tile
    assert tile(8192, 4096, 8) == 256              # the headline: 4096 stereo frames
    assert tile(8192, 384, 8) == 128               # whole 128-position tiles only
    assert tile(8192, 4100, 8) == 0                # not wave-typed: n % 128 != 0
    assert tile(0, 4096, 8) == 0 and tile(8192, 4096, 0) == 0 and tile(8192, 4096, 33) == 0
    # the cases tests/test_gpu_k1_long_tile.py relies on
    assert tile(4162, 256, 8) == 256 and tile(4162, 384, 8) == 128 and tile(16, 768, 8) == 256


def test_autocorr_tile_override_is_read_per_call():
    """FHIP_WT_TILE=128 keeps the 128 form; the switch is read on every call, not once per process (a child, so
    that the C runtime's environment is the one that changes)."""
    code = textwrap.dedent("""
        import ctypes, os, sys
        sys.path.insert(0, %r)
        import flake_amd
        lib = flake_amd.load_library()
        libc = ctypes.CDLL(None)
        a = lib.fhip_autocorr_tile(8192, 4096, 8)
        libc.setenv(b"FHIP_WT_TILE", b"128", 1)
        b = lib.fhip_autocorr_tile(8192, 4096, 8)
        c = lib.fhip_autocorr_tile(8192, 4100, 8)
        libc.unsetenv(b"FHIP_WT_TILE")
        d = lib.fhip_autocorr_tile(8192, 4096, 8)
        print("TILES", a, b, c, d)
    """ % ROOT)
    env = {k: v for k, v in os.environ.items() if k not in ("FHIP_WT_TILE", "FHIP_AC_KERNEL")}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "TILES 256 128 0 256" in r.stdout, r.stdout
