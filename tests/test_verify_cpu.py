"""K5's ABI (no GPU needed) and the frame writer its GPU tests stand on, against the oracle decoder."""
import ctypes as C
import re

import numpy as np

import flake_amd
import flacgen
from test_abi import ROOT, declared


def test_verify_symbols_declared_and_exported():
    lib = flake_amd.load_library()
    names = declared("flakehip.h", "fhip_")
    for n in ("fhip_verify_frames_dev", "fhip_verify_frames", "fhip_set_verify"):
        assert n in names and n in flake_amd.ABI_SYMBOLS
        assert hasattr(lib, n)
    assert hasattr(flake_amd.load_host_library(), "flake_amd_set_verify")
    assert "flake_amd_set_verify" in declared("flake_amd.h", "flake_amd_")


def test_verify_struct_layouts_match_header():
    assert C.sizeof(flake_amd.VerifyIn) == 8 + 8 + 8 + 8 + 8 + 8 + 8
    assert C.sizeof(flake_amd.VerifyOut) == 16
    assert flake_amd.VERIFY_REC_DTYPE.itemsize == 16
    txt = open(f"{ROOT}/include/flakehip.h").read()
    body = re.search(r"typedef struct fhip_verify_in \{(.*?)\} fhip_verify_in;", txt, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in flake_amd.VerifyIn._fields_]
    codes = dict(re.findall(r"FHIP_VERIFY_(\w+) = (\d+)", txt))
    assert [codes[k] for k in flake_amd.VERIFY_STATUS] == [str(i) for i in range(9)]


def test_strerror_verify():
    lib = flake_amd.load_library()
    assert flake_amd.E_VERIFY == -6
    assert lib.fhip_strerror(-6) and lib.fhip_strerror(-6) != lib.fhip_strerror(-99)
    assert lib.fhip_set_verify(None, 1) == flake_amd.E_INVALID


def test_flacgen_frames_decode_to_their_pcm(decoder):
    """Every form in the catalogue: the oracle decoder reproduces the PCM and the CRCs hold."""
    names = set()
    for name, pcm, fr, bps, sr, nch in flacgen.catalogue():
        got, sizes = decoder.decode(np.frombuffer(fr, np.uint8), nch, bps, len(pcm) + 16)
        assert np.array_equal(got, pcm), name
        assert list(sizes) == [len(pcm)]
        names.add(name)
    for need in ("constant", "verbatim", "fixed0", "fixed4", "lpc1", "lpc32", "rice2", "escape", "escape_raw0",
                 "wasted", "ch_independent", "ch8", "ch9", "ch10", "bs_explicit8", "bs_explicit16", "sr_khz",
                 "sr_hz", "sr_tens"):
        assert need in names


def test_flacgen_covers_escape_width_zero_and_rice2():
    for name, pcm, fr, bps, sr, nch in flacgen.catalogue():
        if name == "escape_raw0":
            # partition 0: FIXED 1 residuals of a constant run -- escape code 15 then raw width 0
            w = flacgen.BitWriter()
            flacgen.put_residual(w, [0] * 287 + [1] * 288 * 3, 1152, 1, 0, 2, escape=(0,))
            assert w.bits[6:15] == [1, 1, 1, 1, 0, 0, 0, 0, 0]


def test_flacgen_utf8_numbers(decoder):
    lens = []
    for first, pcm, fr in flacgen.utf8_catalogue():
        got, _ = decoder.decode(np.frombuffer(fr, np.uint8), 1, 16, len(pcm) + 16)
        assert np.array_equal(got, pcm)
        lens.append(len(flacgen.utf8(first)))
    assert lens == [5, 6, 7, 7]
    assert flacgen.utf8(0x7F) == b"\x7f" and flacgen.utf8(0x80) == b"\xc2\x80"


def test_flacgen_crcs_match_the_oracle(oracle):
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8)
        assert flacgen.crc8(bytes(a)) == oracle.crc8(a)
        assert flacgen.crc16(bytes(a)) == oracle.crc16(a)
