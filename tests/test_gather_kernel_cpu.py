"""K9's kernel (k9_gather.hip): it is there and compiles for gfx950 without scratch, without spills and without AGPRs;
K5's and K7's register and LDS figures are what test_index_kernel_cpu.py's BEFORE table holds (K9 shares nothing with
them, and adding it must not move what they compile to); and the new symbols of both libraries and of the Python view
are there.  Runs without a GPU.  The figures are printed (pytest -s) and recorded in DESIGN.md."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flake_amd  # noqa: E402
from flake_amd import build as fb  # noqa: E402
from test_index_kernel_cpu import BEFORE, named  # noqa: E402

needs_hipcc = pytest.mark.skipif(not os.path.exists(fb.HIPCC), reason="needs hipcc")


@needs_hipcc
def test_k9_no_scratch_no_spills_no_agprs():
    kernels = named("k9_gather.hip")
    hit = [(n, r) for n, r in kernels.items() if "::k_gather_spans(" in n]
    assert len(kernels) == 1 and len(hit) == 1, sorted(kernels)
    name, res = hit[0]
    print(f"k_gather_spans: {res['VGPRs']} VGPRs, {res['TotalSGPRs']} SGPRs, {res['LDS Size [bytes/block]']} bytes of LDS, "
          f"{res['Occupancy [waves/SIMD]']} waves per SIMD")
    assert res["ScratchSize [bytes/lane]"] == 0, (name, res)
    assert res["VGPRs Spill"] == 0 and res["SGPRs Spill"] == 0, (name, res)
    assert res.get("AGPRs", 0) == 0, (name, res)
    assert res["LDS Size [bytes/block]"] == 0, (name, res)
    # nothing but latency hiding fills the machine for a copy: the registers must admit full occupancy
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


def test_the_kernel_is_built_into_the_library():
    assert "csrc/k9_gather.hip" in fb.HIP_SRCS
    assert "host/flake_recode_set.c" in fb.HOST_DECODE_SRCS and "host/recode_plan.h" in fb.HOST_DEPS
    text = open(os.path.join(fb.PKG, "csrc", "k9_gather.hip")).read()
    assert re.search(r"__global__[^\n]*\bk_gather_spans\s*\(", text)


HIP_NEW = ("fhip_gather_spans_dev", "fhip_frames_packed_gather", "fhip_decode_frames_segments_keep")
HOST_NEW = ("flake_amd_recode_set_open", "flake_amd_recode_set_frames", "flake_amd_recode_set_out_bound",
            "flake_amd_recode_set_finish", "flake_amd_recode_set_get_streaminfo", "flake_amd_recode_set_failed",
            "flake_amd_recode_set_device_batches", "flake_amd_recode_set_enable_verify", "flake_amd_recode_set_last_error",
            "flake_amd_recode_set_close")


def test_abi_symbols_and_struct_sizes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    header = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    for n in HIP_NEW:
        assert n in flake_amd.ABI_SYMBOLS and hasattr(lib, n), n
        assert f"FHIP_API int {n}(fhip_ctx *ctx, " in header, n
    host_header = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    for n in HOST_NEW:
        assert hasattr(host, n), n
        assert re.search(r"FLAKE_AMD_API [^;]*\b" + n + r"\(", host_header), n
    # fhip_gather_piece: two int32, two int64
    assert flake_amd.GATHER_PIECE_DTYPE.itemsize == 24
    assert [flake_amd.GATHER_PIECE_DTYPE.fields[k][1] for k in ("src_buf", "count", "src", "dst")] == [0, 4, 8, 16]
    for n in ("recode_runs", "finish", "streaminfo", "streaminfo_bytes", "failed", "device_batches"):
        assert hasattr(flake_amd.RecodeSet, n), n
    assert hasattr(flake_amd.Encoder, "gather_spans_dev") and hasattr(flake_amd.Encoder, "frames_packed_gather")


def test_null_handles_are_errors_not_crashes():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    assert lib.fhip_gather_spans_dev(None, None, 0, None, 0, None, 0, None, 0) == flake_amd.E_INVALID
    assert lib.fhip_frames_packed_gather(None, None, None, None, 0, None, 0, None, 0) == flake_amd.E_INVALID
    assert lib.fhip_decode_frames_segments_keep(None, None, None, None, None) == flake_amd.E_INVALID
    assert host.flake_amd_recode_set_frames(None, 0, None, None, None, 0, None, None, 0, None, None, 0, None) == -1
    assert host.flake_amd_recode_set_finish(None, None, 0, None, None, 0, None) == -1
    assert host.flake_amd_recode_set_out_bound(None, 0, None, None) == -1
    assert host.flake_amd_recode_set_get_streaminfo(None, 0, None) == -1
    assert host.flake_amd_recode_set_failed(None, 0, None, None) == -1
    host.flake_amd_recode_set_close(None)


def test_open_refusals_that_need_no_device():
    """What flake_amd_recode_set_open refuses before it opens a handle."""
    host = flake_amd.load_host_library()
    si = flake_amd.HostStreaminfo(min_block_size=64, max_block_size=64, sample_rate=44100, channels=2, bits_per_sample=16)

    def refused(flags=0, level=5, block_size=None, **fmt):
        ctx = flake_amd.HostContext(channels=fmt.get("channels", 2), sample_rate=fmt.get("sample_rate", 44100),
                                    bits_per_sample=fmt.get("bits_per_sample", 16))
        ctx.params.compression = level
        assert host.flake_amd_set_defaults(C.byref(ctx.params)) == 0
        if block_size:
            ctx.params.block_size = block_size
        assert not host.flake_amd_recode_set_open(C.byref(si), C.byref(ctx), 3, flags)
        return host.flake_amd_recode_set_last_error(None).decode()

    assert "MD5_HOST" in refused(flags=flake_amd.SET_MD5_HOST)
    assert "unknown flags" in refused(flags=64)
    assert "16384" in refused(block_size=16385)
    for fmt in (dict(channels=1), dict(sample_rate=48000), dict(bits_per_sample=24)):
        assert "source format" in refused(**fmt)
    assert "variable block size" in refused(level=10)                       # levels 9-12 need SET_VBS
    assert "FLAKE_AMD_SET_VBS needs" in refused(level=5, flags=flake_amd.SET_VBS)       # and only they take it
