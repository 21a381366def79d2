"""K8's kernels (k8_index.hip): every one is there and compiles for gfx950 without scratch, without spills and without
AGPRs; and K5's and K7's register and LDS figures are what they were before K8 came (K8 shares flac_header.h's tables
and flac_parse.h's CRC-16 and scan with them, and sharing must not move what they compile to).  Runs without a GPU.
The figures are printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402
from test_k3_residency_cpu import _resources  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

K8 = ("k_index_scan<false>", "k_index_scan<true>", "k_index_wgscan", "k_index_walk", "k_index_ranges", "k_index_emit")

# (VGPRs, TotalSGPRs, VGPRs Spill, SGPRs Spill, LDS bytes per block).  k_decode's and the three end kernels' rows are of
# the commit before K8; the other six of the commit that brought flac_frame_pass.h and k7_frame.h and moved their spill
# counts, nothing else (profiles/k5_k7_frame_pass_refactor.txt holds both sides)
BEFORE = {
    "k5_verify.hip": {
        "k_verify(": (108, 106, 0, 10, 52480),
        "k_verify_final(": (4, 15, 0, 0, 0),
        "k_verify_frames<0>(": (128, 106, 14, 117, 12432),
        "k_verify_frames<1>(": (128, 106, 14, 94, 128),
        "k_verify_frames<2>(": (128, 106, 16, 94, 128),
    },
    "k7_decode.hip": {
        "k_decode(": (49, 106, 0, 16, 17120),
        "k_decode_final(": (4, 14, 0, 0, 0),
        "k_decode_seg_final(": (4, 21, 0, 0, 0),
        "k_decode_frames<false>(": (128, 106, 18, 31, 16536),
        "k_decode_frames<true>(": (128, 106, 49, 88, 16536),
    },
}


def named(src):
    found, err = _resources(os.path.join(fb.PKG, "csrc", src))
    out = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip(): v for k, v in found.items()}
    assert out, err[-2000:]
    return out


@needs_hipcc
def test_k8_no_scratch_no_spills_no_agprs():
    kernels = named("k8_index.hip")
    assert len(kernels) == len(K8), sorted(kernels)
    for want in K8:
        hit = [(n, r) for n, r in kernels.items() if "::" + want + "(" in n]
        assert len(hit) == 1, (want, sorted(kernels))
        name, res = hit[0]
        print(f"{want}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, {res['LDS Size [bytes/block]']} bytes of LDS")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)


@needs_hipcc
@pytest.mark.parametrize("src", sorted(BEFORE))
def test_k5_and_k7_compile_to_what_they_did(src):
    kernels = named(src)
    assert len(kernels) == len(BEFORE[src]), sorted(kernels)
    for want, figures in BEFORE[src].items():
        hit = [r for n, r in kernels.items() if "::" + want in n]
        assert len(hit) == 1, (want, sorted(kernels))
        r = hit[0]
        got = (r["VGPRs"], r["TotalSGPRs"], r["VGPRs Spill"], r["SGPRs Spill"], r["LDS Size [bytes/block]"])
        print(f"{want[:-1]}: {got}")
        assert got == figures, (want, got, figures)


def test_abi_symbols_and_struct_sizes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    for n in ("fhip_index_frames_dev", "fhip_index_frames", "fhip_index_geometry"):
        assert n in flake_amd.ABI_SYMBOLS and hasattr(lib, n), n
    for n in ("flake_amd_decode_index", "flake_amd_decode_set_index"):
        assert hasattr(host, n), n
    # fhip_index_in: pointer, int64, pointer, three int32 and padding; fhip_index_out: four pointers
    assert C.sizeof(flake_amd.IndexIn) == 40 and C.sizeof(flake_amd.IndexOut) == 32
    assert flake_amd.IndexIn.frame_cap.offset == 32 and flake_amd.IndexOut.range_variable.offset == 24
    header = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    for n in ("fhip_index_frames_dev", "fhip_index_frames"):
        assert f"FHIP_API int {n}(fhip_ctx *ctx, const fhip_index_in *in, const fhip_index_out *out);" in header
    assert hasattr(flake_amd.HostDecoder, "index") and hasattr(flake_amd.DecodeSet, "index")
