"""K12's kernel (k12_rows_in.hip) and the encode-rows entries without a GPU: every instance compiles for gfx950 without
scratch, without spills, without AGPRs and without LDS; the file is part of the build; the new symbols are in both
libraries, both headers and the Python view; flakehip.h includes the new header; null handles are refused.  The figures
are printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402
from test_index_kernel_cpu import named  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")

HIP_NEW = ("fhip_pcm_from_rows_dev", "fhip_frames_packed_from_rows")


@needs_hipcc
def test_k12_no_scratch_no_spills_no_agprs_no_lds():
    kernels = named("k12_rows_in.hip")
    hit = {n: r for n, r in kernels.items() if "::k_rows_to_pcm<" in n}
    # one instance per format and channel count, nothing else
    assert len(kernels) == len(hit) == 3 * 8, sorted(kernels)
    for fmt in range(3):
        for ch in range(1, 9):
            assert any(re.search(r"k_rows_to_pcm<%d, %d>" % (fmt, ch), n) for n in hit), (fmt, ch, sorted(hit))
    for name, res in sorted(hit.items()):
        inst = re.search(r"k_rows_to_pcm<[^>]*>", name).group(0)
        print(f"{inst}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, {res['LDS Size [bytes/block]']} bytes of LDS, "
              f"{res['Occupancy [waves/SIMD]']} waves per SIMD")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)
        assert res["LDS Size [bytes/block]"] == 0, (name, res)
        # nothing but latency hiding fills the machine for a conversion: the registers must admit full occupancy
        assert res["Occupancy [waves/SIMD]"] == 8, (name, res)


def test_the_kernel_is_built_into_the_library():
    assert "csrc/k12_rows_in.hip" in fb.HIP_SRCS
    assert "../include/flakehip_rows_in.h" in fb.HIP_HDRS and "host/rows_plan.h" in fb.HOST_DEPS
    text = open(os.path.join(fb.PKG, "csrc", "k12_rows_in.hip")).read()
    assert re.search(r"__global__[^;{]*\bk_rows_to_pcm\s*\(", text)
    assert 'note_launch("k_rows_to_pcm")' in text
    assert "__shared__" not in text
    hdr = open(os.path.join(fb.PKG, "csrc", "kernels.h")).read()
    assert "struct RowsInArgs" in hdr and "launch_rows_to_pcm(" in hdr
    assert '"k_rows_to_pcm"' in open(os.path.join(fb.PKG, "csrc", "api.hip")).read()       # the profiling slot


def test_symbols_headers_and_the_python_view():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    main_h = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    rows_h = open(os.path.join(ROOT, "include", "flakehip_rows_in.h")).read()
    host_h = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    assert '#include "flakehip_rows_in.h"' in main_h
    assert main_h.index('#include "flakehip_held.h"') < main_h.index('#include "flakehip_rows_in.h"')
    assert tuple(flake_amd.ROWS_IN_ABI_SYMBOLS) == HIP_NEW
    for n in HIP_NEW:
        assert hasattr(lib, n), n
        assert f"FHIP_API int {n}(fhip_ctx *ctx, " in rows_h, n
        # declared in the new header only: flakehip.h's own list of entries is what other tests hold to their cases
        assert not re.search(r"FHIP_API[^;]*\b%s\s*\(" % n, main_h), n
    for word in ("} fhip_rows_in;", "} fhip_row_piece;", '"k_rows_to_pcm"'):
        assert word in rows_h, word
    assert hasattr(host, "flake_amd_set_encode_rows")
    assert re.search(r"FLAKE_AMD_API long long flake_amd_set_encode_rows\(FlakeAmdSet \*g,", host_h)
    assert C.sizeof(flake_amd.RowsIn) == 24 and flake_amd.RowsIn.row_len.offset == 16
    assert C.sizeof(flake_amd.RowPiece) == 24
    assert [getattr(flake_amd.RowPiece, k).offset for k in ("row", "count", "col", "dst")] == [0, 4, 8, 16]
    assert [flake_amd.ROW_PIECE_DTYPE.fields[k][1] for k in ("row", "count", "col", "dst")] == [0, 4, 8, 16]
    t = flake_amd.row_pieces([(2, 5, 7, 11)])
    assert (t["row"][0], t["col"][0], t["dst"][0], t["count"][0]) == (2, 5, 7, 11)
    assert hasattr(flake_amd.Encoder, "pcm_from_rows_dev") and hasattr(flake_amd.Encoder, "frames_packed_from_rows")
    assert hasattr(flake_amd.StreamSet, "encode_rows")


def test_null_handles_are_errors_not_crashes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    ri = flake_amd.RowsIn(None, 1, 0, 1)
    assert lib.fhip_pcm_from_rows_dev(None, None, 0, C.byref(ri), None, 0) == flake_amd.E_INVALID
    assert lib.fhip_pcm_from_rows_dev(None, None, 0, None, None, 0) == flake_amd.E_INVALID
    assert lib.fhip_frames_packed_from_rows(None, None, None, None, None, 0) == flake_amd.E_INVALID
    assert host.flake_amd_set_encode_rows(None, None, 0, 0, 0, None, None, None, 0, None, None) == -1
