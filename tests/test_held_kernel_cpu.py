"""K11's kernels (k11_held.hip): every one is there and compiles for gfx950 without scratch, without spills and without
AGPRs, the copy and the two per-frame passes with no LDS and the scan with nothing beyond its wave totals; K5's and K7's
register and LDS figures are what test_index_kernel_cpu.py's BEFORE table holds, and K8, K9 and K10 still compile as
their own tests demand (K11 shares kernels.h and flac_header.h with them, and adding it must not move what they compile
to); and the new symbols of both libraries and of the Python view are there.  Runs without a GPU.  The figures are
printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402
from test_index_kernel_cpu import BEFORE, K8, named  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

# kernel -> the most LDS it may hold, in bytes per block
K11 = {"k_frame_heads": 0, "k_frame_offsets": 0, "k_gather_offsets": 16 * 8, "k_gather_frames": 0}


@needs_hipcc
def test_k11_no_scratch_no_spills_no_agprs():
    kernels = named("k11_held.hip")
    assert len(kernels) == len(K11), sorted(kernels)
    for want, lds in K11.items():
        hit = [(n, r) for n, r in kernels.items() if "::" + want + "(" in n]
        assert len(hit) == 1, (want, sorted(kernels))
        name, res = hit[0]
        print(f"{want}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, {res['LDS Size [bytes/block]']} bytes of LDS, "
              f"{res['Occupancy [waves/SIMD]']} waves per SIMD")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)
        assert res["LDS Size [bytes/block]"] <= lds, (name, res)
        # latency hiding is all that fills the machine for these: the registers must admit full occupancy
        assert res["Occupancy [waves/SIMD]"] == 8, (name, res)


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


@needs_hipcc
@pytest.mark.parametrize("src,count", [("k8_index.hip", len(K8)), ("k9_gather.hip", 1), ("k10_rows.hip", 3)])
def test_k8_k9_k10_keep_their_kernels_clean(src, count):
    kernels = named(src)
    assert len(kernels) == count, sorted(kernels)
    for name, res in kernels.items():
        print(f"{name.split('::')[-1].split('(')[0]}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, "
              f"{res['LDS Size [bytes/block]']} bytes of LDS")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)


def test_the_kernels_are_built_into_the_library():
    assert "csrc/k11_held.hip" in fb.HIP_SRCS and "host/held_plan.h" in fb.HOST_DEPS
    text = open(os.path.join(fb.PKG, "csrc", "k11_held.hip")).read()
    for k in K11:
        assert re.search(r"__global__[^\n]*\b" + k + r"\s*\(", text), k
        assert f'note_launch("{k}")' in text, k
    # the predicate is called, not restated
    assert "flac_header_ok(&a.fmt" in text and "crc8" not in text


HIP_NEW = ("fhip_frame_heads_dev", "fhip_gather_frames_dev", "fhip_decode_frames_windows_held",
           "fhip_decode_frames_windows_rows_held", "fhip_hold_frames")
HOST_NEW = ("flake_amd_decode_set_hold", "flake_amd_decode_set_hold_add", "flake_amd_decode_set_held_windows",
            "flake_amd_decode_set_held_windows_rows", "flake_amd_decode_set_held_info", "flake_amd_decode_set_held_stats")


def test_abi_symbols_and_struct_sizes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    # the held-streams entries have a header of their own, which flakehip.h includes
    assert '#include "flakehip_held.h"' in open(os.path.join(ROOT, "include", "flakehip.h")).read()
    header = open(os.path.join(ROOT, "include", "flakehip_held.h")).read()
    for n in HIP_NEW:
        assert n in flake_amd.HELD_ABI_SYMBOLS and hasattr(lib, n), n
        assert f"FHIP_API int {n}(fhip_ctx *ctx, " in header, n
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(fhip_\w+)\s*\(", plain))) == sorted(flake_amd.HELD_ABI_SYMBOLS)
    assert not set(flake_amd.HELD_ABI_SYMBOLS) & set(flake_amd.ABI_SYMBOLS)
    assert "} fhip_frame_head;" in header
    host_header = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    for n in HOST_NEW:
        assert hasattr(host, n), n
        assert re.search(r"FLAKE_AMD_API [^;]*\b" + n + r"\(", host_header), n
    # fhip_frame_head: a uint64 and two int32
    assert flake_amd.FRAME_HEAD_DTYPE.itemsize == 16
    assert [flake_amd.FRAME_HEAD_DTYPE.fields[k][1] for k in ("number", "n", "flags")] == [0, 8, 12]
    for n in ("hold", "hold_add", "held_windows", "held_windows_rows", "held_info", "held_stats"):
        assert hasattr(flake_amd.DecodeSet, n), n
    for n in ("frame_heads_dev", "gather_frames_dev", "decode_frames_windows_held", "decode_frames_windows_rows_held"):
        assert hasattr(flake_amd.Encoder, n), n


def test_null_handles_are_errors_not_crashes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    assert lib.fhip_frame_heads_dev(None, None, 0, None, None, 0, 0, None) == flake_amd.E_INVALID
    assert lib.fhip_gather_frames_dev(None, None, 0, None, None, 0, None, None, 0) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_windows_held(None, None, 0, None, None, 0, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_windows_rows_held(None, None, 0, None, None, 0, None, None, None, None, None,
                                                    None) == flake_amd.E_INVALID
    assert lib.fhip_hold_frames(None, None, None) == flake_amd.E_INVALID
    assert host.flake_amd_decode_set_hold(None, 1) == -1
    assert host.flake_amd_decode_set_hold_add(None, 0, None, None, 0, None, None) == -1
    assert host.flake_amd_decode_set_held_windows(None, 0, None, None, None, None, 4, 0, None, None, None) == -1
    assert host.flake_amd_decode_set_held_windows_rows(None, 0, None, None, None, None, 0, 1, None, None, None) == -1
    assert host.flake_amd_decode_set_held_info(None, 0, None, None, None) == -1
    assert host.flake_amd_decode_set_held_stats(None, None) == -1
