"""Window rows (K10: fhip_rows_from_segments_dev, fhip_rows_zero_dev, fhip_decode_frames_windows_rows,
flake_amd_decode_set_windows_rows) without a GPU: the entries are declared in the headers and exported by both
libraries, the kernel file is part of the build, null handles are refused and the kernel compiles for gfx950 without
scratch and without spills."""
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
from test_k3_residency_cpu import _resources  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

FHIP = ("fhip_rows_from_segments_dev", "fhip_rows_zero_dev", "fhip_decode_frames_windows_rows")


def test_entries_are_declared_and_exported():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    hip_h = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    host_h = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    for n in FHIP:
        assert n in flake_amd.ABI_SYMBOLS and hasattr(lib, n), n
        assert re.search(r"FHIP_API int %s\(fhip_ctx \*ctx," % n, hip_h), n
    for word in ("FHIP_ROWS_I32 0", "FHIP_ROWS_I16 1", "FHIP_ROWS_F32 2", "} fhip_rows_out;", '"k_window_rows"'):
        assert word in hip_h, word
    assert hasattr(host, "flake_amd_decode_set_windows_rows")
    assert re.search(r"FLAKE_AMD_API long long flake_amd_decode_set_windows_rows\(FlakeAmdDecodeSet \*g,", host_h)
    for word in ("FLAKE_AMD_ROWS_I32 0", "FLAKE_AMD_ROWS_I16 1", "FLAKE_AMD_ROWS_F32 2"):
        assert word in host_h, word
    assert (flake_amd.ROWS_I32, flake_amd.ROWS_I16, flake_amd.ROWS_F32) == (0, 1, 2)
    assert C.sizeof(flake_amd.RowsOut) == 24 and flake_amd.RowsOut.row_len.offset == 16
    assert hasattr(flake_amd.DecodeSet, "decode_windows_rows")
    for name in ("rows_from_segments_dev", "rows_zero_dev", "decode_frames_windows_rows"):
        assert hasattr(flake_amd.Encoder, name)


def test_the_kernel_file_is_built():
    assert "csrc/k10_rows.hip" in fb.HIP_SRCS
    text = open(os.path.join(fb.PKG, "csrc", "k10_rows.hip")).read()
    assert 'note_launch("k_window_rows")' in text
    hdr = open(os.path.join(fb.PKG, "csrc", "kernels.h")).read()
    assert "struct WindowRowsArgs" in hdr and "launch_window_rows(" in hdr


def test_null_handles_are_errors_not_crashes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    ro = flake_amd.RowsOut(None, 1, 0, 1)
    assert lib.fhip_rows_from_segments_dev(None, None, 0, 0, None, None, None, None, None, C.byref(ro)) == flake_amd.E_INVALID
    assert lib.fhip_rows_from_segments_dev(None, None, 0, 0, None, None, None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_rows_zero_dev(None, C.byref(ro), 0, 1) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_windows_rows(None, None, None, None, None, None, None, None) == flake_amd.E_INVALID
    assert host.flake_amd_decode_set_windows_rows(None, 0, None, None, 0, None, None, None, None, None,
                                                  flake_amd.ROWS_F32, 16, None, None, None) == -1


@needs_hipcc
def test_the_kernel_compiles_lean():
    found, err = _resources(os.path.join(fb.PKG, "csrc", "k10_rows.hip"))
    named = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip(): v for k, v in found.items()}
    rows = {n: r for n, r in named.items() if "k_window_rows<" in n}
    assert len(rows) == 3 and len(named) == 3, (sorted(named), err[-2000:])      # one instance per format, nothing else
    for n, r in sorted(rows.items()):
        print(f"{n}: {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs, {r['LDS Size [bytes/block]']} bytes of LDS, "
              f"{r['ScratchSize [bytes/lane]']} bytes of scratch, occupancy {r['Occupancy [waves/SIMD]']}")
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert r["LDS Size [bytes/block]"] == 8 * 512 * 4, (n, r)                # one tile of eight channels
        assert r["Occupancy [waves/SIMD]"] == 8, (n, r)
