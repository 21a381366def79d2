"""K13's kernel (k13_span_rows.hip) and the span-rows entries without a GPU: every instance compiles for gfx950 without
scratch, without spills, without AGPRs and with no more LDS than K10's 16 KiB; the file is part of the build; the new
symbols are in both libraries, in the new header only and in the Python view; flakehip.h includes the new header behind
flakehip_rows_in.h; null handles are refused.  The figures are printed (pytest -s) and recorded in DESIGN.md."""
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

HIP_NEW = ("fhip_span_rows_from_segments_dev", "fhip_decode_frames_windows_spans", "fhip_decode_frames_windows_spans_held")
HOST_NEW = ("flake_amd_span_rows_count", "flake_amd_decode_set_span_rows", "flake_amd_decode_set_held_span_rows")


@needs_hipcc
def test_k13_no_scratch_no_spills_no_agprs_lds_of_k10():
    kernels = named("k13_span_rows.hip")
    hit = {n: r for n, r in kernels.items() if "::k_span_rows<" in n}
    # one instance per format, nothing else: one body for every channel count, row_len and hop
    assert len(kernels) == len(hit) == 3, sorted(kernels)
    for fmt in range(3):
        assert any(re.search(r"k_span_rows<%d>" % fmt, n) for n in hit), (fmt, sorted(hit))
    for name, res in sorted(hit.items()):
        inst = re.search(r"k_span_rows<[^>]*>", name).group(0)
        print(f"{inst}: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, {res['LDS Size [bytes/block]']} bytes of LDS, "
              f"{res['Occupancy [waves/SIMD]']} waves per SIMD")
        assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
        assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
        assert res.get("AGPRs", 0) == 0, (name, res)
        assert 0 < res["LDS Size [bytes/block]"] <= 16384, (name, res)


def test_the_kernel_is_built_into_the_library():
    assert "csrc/k13_span_rows.hip" in fb.HIP_SRCS
    assert fb.HIP_SRCS.index("csrc/k13_span_rows.hip") < fb.HIP_SRCS.index("csrc/api.hip")
    assert "../include/flakehip_spans.h" in fb.HIP_HDRS and "../include/flakehip_spans.h" in fb.HOST_DEPS
    assert "host/span_rows_plan.h" in fb.HOST_DEPS
    text = open(os.path.join(fb.PKG, "csrc", "k13_span_rows.hip")).read()
    assert re.search(r"__global__[^;{]*\bk_span_rows\s*\(", text)
    assert 'note_launch("k_span_rows")' in text
    hdr = open(os.path.join(fb.PKG, "csrc", "kernels.h")).read()
    assert "struct SpanRowsArgs" in hdr and "launch_span_rows(" in hdr
    assert '"k_span_rows"' in open(os.path.join(fb.PKG, "csrc", "api.hip")).read()         # the profiling slot


def test_symbols_headers_and_the_python_view():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    main_h = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    held_h = open(os.path.join(ROOT, "include", "flakehip_held.h")).read()
    rows_h = open(os.path.join(ROOT, "include", "flakehip_rows_in.h")).read()
    span_h = open(os.path.join(ROOT, "include", "flakehip_spans.h")).read()
    host_h = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    assert '#include "flakehip_spans.h"' in main_h
    assert (main_h.index('#include "flakehip_held.h"') < main_h.index('#include "flakehip_rows_in.h"')
            < main_h.index('#include "flakehip_spans.h"'))
    assert tuple(flake_amd.SPANS_ABI_SYMBOLS) == HIP_NEW
    plain = re.sub(r"/\*.*?\*/", "", span_h, flags=re.S)
    assert sorted(set(re.findall(r"\b(fhip_\w+)\s*\(", plain))) == sorted(HIP_NEW)
    for other in (flake_amd.ABI_SYMBOLS, flake_amd.HELD_ABI_SYMBOLS, flake_amd.ROWS_IN_ABI_SYMBOLS):
        assert not set(HIP_NEW) & set(other)
    for n in HIP_NEW:
        assert hasattr(lib, n), n
        assert f"FHIP_API int {n}(fhip_ctx *ctx, " in span_h, n
        # declared in the new header only: the other headers' own lists of entries are what other tests hold to their cases
        for text in (main_h, held_h, rows_h):
            assert not re.search(r"FHIP_API[^;]*\b%s\s*\(" % n, text), n
    for word in ("} fhip_span_rows;", '"k_span_rows"'):
        assert word in span_h, word
    for n in HOST_NEW:
        assert hasattr(host, n), n
        assert re.search(r"FLAKE_AMD_API long long %s\(" % n, host_h), n
    assert C.sizeof(flake_amd.SpanRows) == 48
    assert [getattr(flake_amd.SpanRows, k).offset for k in ("seg_row0", "seg_nrows", "seg_pos", "hop", "tile_first", "ntiles")] \
        == [0, 8, 16, 24, 32, 40]
    assert hasattr(flake_amd.Encoder, "span_rows_from_segments_dev")
    assert hasattr(flake_amd.DecodeSet, "decode_span_rows") and hasattr(flake_amd.DecodeSet, "held_span_rows")


def test_span_rows_count_is_pure():
    c = flake_amd.span_rows_count
    assert [c(0, 4, 2), c(1, 4, 2), c(4, 4, 2), c(5, 4, 2), c(10, 4, 2), c(10, 4, 4), c(10, 4, 7)] == [0, 1, 1, 2, 4, 3, 2]
    assert [c(-1, 4, 2), c(4, 0, 2), c(4, 4, 0), c(4, 4, 2 ** 31)] == [-1] * 4
    assert c(4, 4, 2 ** 31 - 1) == 1


def test_null_handles_are_errors_not_crashes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    sp = flake_amd.SpanRows(None, None, None, 1, None, 0)
    ro = flake_amd.RowsOut(None, 1, 0, 1)
    assert lib.fhip_span_rows_from_segments_dev(None, None, 0, 0, None, None, None, C.byref(sp), C.byref(ro)) == flake_amd.E_INVALID
    assert lib.fhip_span_rows_from_segments_dev(None, None, 0, 0, None, None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_windows_spans(None, None, None, None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_windows_spans_held(None, None, 0, None, None, 0, None, None, None, None, None) == flake_amd.E_INVALID
    assert host.flake_amd_decode_set_span_rows(None, 0, None, None, 0, None, None, None, None, 1, None, 0, 1, 0, None, None,
                                               None, None) == -1
    assert host.flake_amd_decode_set_held_span_rows(None, 0, None, None, None, 1, None, 0, 1, 0, None, None, None, None) == -1
