"""Windows (fhip_decode_frames_windows, flake_amd_decode_set_windows) without a GPU: the new symbols exist in both
libraries and refuse null handles, the headers document them, and the window instance of K7's frame kernel is no
heavier than the existing one.

k_decode_windows (k7_decode_windows.hip) is k7_frame.h's decode_frame_window, k_decode's text with the clip in its
write-out; the twin it is held to is k_decode (k7_decode.hip), under the same flags and the same compiler, in this test
run -- not a number written down here.  Residency of k_decode is LDS-limited, so the window
instance must have exactly its LDS; and no more scratch."""
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


def test_abi_symbols_and_null_handles():
    lib, host = flake_amd.load_library(), flake_amd.load_host_library()
    for n in ("fhip_decode_frames_windows_dev", "fhip_decode_frames_windows"):
        assert n in flake_amd.ABI_SYMBOLS and hasattr(lib, n), n
        assert getattr(lib, n)(None, None, None, None, None) == flake_amd.E_INVALID
    assert C.sizeof(flake_amd.DecodeWindows) == 16 and flake_amd.DecodeWindows.seg_take.offset == 8
    for n in ("flake_amd_decode_set_windows", "flake_amd_read_seektable", "flake_amd_seek_lookup"):
        assert hasattr(host, n), n
    assert host.flake_amd_decode_set_windows(None, 0, None, None, 0, None, None, None, None, None, 4, 0, None, None, None) == -1
    assert host.flake_amd_read_seektable(None, 18, None, 0) == -1 and host.flake_amd_seek_lookup(None, 0, 0) == -1
    for name in ("decode_frames_windows", "decode_frames_windows_dev"):
        assert hasattr(flake_amd.Encoder, name)
    assert hasattr(flake_amd.DecodeSet, "decode_windows") and flake_amd.SEEK_POINT_DTYPE.itemsize == 24


def test_headers_document_the_entries():
    hip = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    for n in ("fhip_decode_frames_windows_dev", "fhip_decode_frames_windows"):
        assert re.search(r"FHIP_API int %s\(fhip_ctx \*ctx, const fhip_decode_in \*in, const fhip_decode_segments \*segs,\s*"
                         r"const fhip_decode_windows \*win, const fhip_decode_out \*out\);" % n, hip), n
    for word in ("seg_skip", "seg_take", '"k_decode_frames windows"', '"k_decode windows"'):
        assert word in hip, word
    host = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    for n in ("flake_amd_decode_set_windows", "flake_amd_read_seektable", "flake_amd_seek_lookup", "FlakeAmdSeekPoint"):
        assert n in host, n


def named(src):
    found, err = _resources(os.path.join(fb.PKG, "csrc", src))
    out = {subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip(): v for k, v in found.items()}
    assert out, err[-2000:]
    return out


@needs_hipcc
def test_the_window_instance_is_no_heavier_than_its_twin():
    twin = [r for n, r in named("k7_decode.hip").items() if "::k_decode(" in n]
    wins = named("k7_decode_windows.hip")
    assert len(wins) == 2, sorted(wins)                                   # the header pass and the frame pass, nothing else
    win = [r for n, r in wins.items() if "::k_decode_windows(" in n]
    hdr = [r for n, r in wins.items() if "::k_decode_frames_windows(" in n]
    assert len(twin) == 1 and len(win) == 1 and len(hdr) == 1
    t, w = twin[0], win[0]
    for what, r in (("k_decode", t), ("k_decode_windows", w), ("k_decode_frames_windows", hdr[0])):
        print(f"{what}: {r['VGPRs']} VGPRs, {r['TotalSGPRs']} SGPRs, {r['LDS Size [bytes/block]']} bytes of LDS, "
              f"{r['ScratchSize [bytes/lane]']} bytes of scratch")
    assert w["LDS Size [bytes/block]"] == t["LDS Size [bytes/block]"], (w, t)
    assert w["ScratchSize [bytes/lane]"] <= t["ScratchSize [bytes/lane]"], (w, t)
    assert w["VGPRs Spill"] == 0 and w["Occupancy [waves/SIMD]"] >= t["Occupancy [waves/SIMD]"], (w, t)
