"""The frame-header predicate (flake_amd/csrc/flac_header.h) on its own: one source for the host layer (gcc, C99) and
for K8 (hipcc, C++17), so a host program (tools/flac_header_dump.c) is built from it as C99, as C++17 and with
-fsanitize=address,undefined, and all three must print the same verdicts for a catalogue of headers -- the verdicts of
the parser below, which is written from the FLAC format and reads none of the C.  Every case lies in an allocation of
exactly its `avail` bytes: the sanitized build reports a read at or past avail.  Runs without a GPU.
tests/test_gpu_index.py puts the same catalogue through K8."""
import os
import subprocess

import pytest

import flacgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flake_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "flac_header_dump.c")

BASE = (2, 16, 48000, 0)               # channels, bits per sample, rate, max block size (0: no limit)

RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
SIZES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


# ---- the reference: a frame header as the FLAC format describes it -------------------------------------------

class Short(Exception):
    pass


def reference(fmt, data, avail):
    """(n, vbs, len, number) when data[:avail] begins with a frame header of a stream of this format, else None."""
    channels, bps, rate, max_block = fmt
    data = bytes(data[:avail])
    at = [0]

    def byte():
        if at[0] >= len(data):
            raise Short()
        at[0] += 1
        return data[at[0] - 1]

    try:
        sync = byte() << 8 | byte()
        if sync >> 2 != 0x3FFE or sync & 2:                    # 14 bits of sync, a reserved zero
            return None
        vbs = sync & 1
        b2, b3 = byte(), byte()
        bs_code, sr_code, ch_code, size_code = b2 >> 4, b2 & 15, b3 >> 4, (b3 >> 1) & 7
        if b3 & 1:                                              # a reserved zero
            return None
        if bs_code == 0 or sr_code == 15 or size_code == 3:     # reserved codes
            return None
        if ch_code <= 7:                                        # independent channels
            if channels != ch_code + 1:
                return None
        elif ch_code <= 10:                                     # the three stereo decorrelations
            if channels != 2:
                return None
        else:
            return None
        if size_code and SIZES.get(bps) != size_code:           # 0: as STREAMINFO says
            return None
        if 1 <= sr_code <= 11 and RATES[sr_code] != rate:
            return None
        first = byte()
        lead = 0
        while lead < 8 and first & (0x80 >> lead):
            lead += 1
        if lead == 1 or lead == 8:                              # a continuation byte, or no payload form
            return None
        number = first & (0xFF >> (lead + 1)) if lead else first
        for _ in range(max(lead - 1, 0)):
            c = byte()
            if c >> 6 != 2:
                return None
            number = number << 6 | (c & 63)
        if bs_code == 1:
            n = 192
        elif bs_code <= 5:
            n = 576 * 2 ** (bs_code - 2)
        elif bs_code == 6:
            n = byte() + 1
        elif bs_code == 7:
            n = (byte() << 8 | byte()) + 1
        else:
            n = 256 * 2 ** (bs_code - 8)
        if n > 65535 or (max_block and n > max_block):          # STREAMINFO's block sizes are 16-bit fields
            return None
        if sr_code == 12 and byte() * 1000 != rate:
            return None
        if sr_code == 13 and (byte() << 8 | byte()) != rate:
            return None
        if sr_code == 14 and (byte() << 8 | byte()) * 10 != rate:
            return None
        covered = at[0]
        if byte() != flacgen.crc8(data[:covered]):
            return None
        return n, vbs, at[0], number
    except Short:
        return None


# ---- the catalogue ------------------------------------------------------------------------------------------

def header(bs_code=12, n=None, sr_code=10, rate_field=None, ch_code=1, size_code=4, number=b"\x00", vbs=0, res1=0, res2=0,
           sync=0x3FFE):
    """A header from its raw fields (number: the coded bytes, or an int for flacgen.utf8), its CRC-8 behind it."""
    w = flacgen.BitWriter()
    w.put(14, sync)
    w.put(1, res1)
    w.put(1, vbs)
    w.put(4, bs_code)
    w.put(4, sr_code)
    w.put(4, ch_code)
    w.put(3, size_code)
    w.put(1, res2)
    for b in (flacgen.utf8(number) if isinstance(number, int) else number):
        w.put(8, b)
    if bs_code in (6, 7):
        w.put(8 if bs_code == 6 else 16, n - 1)
    if sr_code in (12, 13, 14):
        w.put(8 if sr_code == 12 else 16, rate_field)
    body = w.tobytes()
    return body + bytes([flacgen.crc8(body)])


def valid_headers():
    """Headers of a BASE stream, every one a header: each block-size, rate, channel and sample-size code the format
    allows it, numbers of one to seven bytes, both strategy bits."""
    out = []
    for vbs in (0, 1):
        for code in (1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15):
            out.append(header(bs_code=code, vbs=vbs))
        out += [header(bs_code=6, n=1, vbs=vbs), header(bs_code=6, n=256, vbs=vbs), header(bs_code=7, n=1, vbs=vbs),
                header(bs_code=7, n=65535, vbs=vbs)]
        out += [header(sr_code=0, vbs=vbs), header(sr_code=12, rate_field=48, vbs=vbs),
                header(sr_code=13, rate_field=48000, vbs=vbs), header(sr_code=14, rate_field=4800, vbs=vbs)]
        out += [header(ch_code=c, vbs=vbs) for c in (8, 9, 10)]
        out.append(header(size_code=0, vbs=vbs))
        out += [header(number=v, vbs=vbs) for v in (0x7F, 0x80, 0x800, 0x10000, 0x200000, 0x4000000, 0x80000000, (1 << 36) - 1)]
        # everything explicit at once: the longest header there is, 16 bytes
        out.append(header(bs_code=7, n=4097, sr_code=13, rate_field=48000, number=(1 << 36) - 2, vbs=vbs))
    return out


def field_cases():
    """(format, header, is it one?): a reserved code, a code that disagrees with the format, and what other formats
    accept.  Each CRC-8 holds, so the field decides."""
    no = [header(bs_code=0), header(sr_code=15), header(res1=1), header(res2=1), header(sync=0x3FFC), header(sync=0x1FFE),
          header(bs_code=7, n=65536)]
    no += [header(sr_code=c) for c in (1, 9, 11)]
    no += [header(sr_code=12, rate_field=44), header(sr_code=13, rate_field=44100), header(sr_code=14, rate_field=4410),
           header(sr_code=14, rate_field=48000)]
    no += [header(ch_code=c) for c in (0, 2, 7, 11, 12, 13, 14, 15)]
    no += [header(size_code=c) for c in (1, 2, 3, 5, 6, 7)]
    no += [header(number=bytes([b])) for b in (0x80, 0xBF, 0xFF)]
    no += [header(number=bytes(b)) for b in ([0xC2, 0x00], [0xC2, 0x40], [0xC2, 0xC0], [0xE1, 0x80, 0x7F],
                                             [0xFE, 0x80, 0x80, 0x80, 0x80, 0xFF, 0x80])]
    out = [(BASE, h, False) for h in no]
    out += [(fmt, header(), False) for fmt in ((1, 16, 48000, 0), (3, 16, 48000, 0), (2, 24, 48000, 0), (2, 16, 44100, 0),
                                               (2, 16, 48000, 4095))]
    out += [((1, 16, 48000, 0), header(ch_code=0), True), ((1, 16, 48000, 0), header(ch_code=8), False),
            ((8, 16, 48000, 0), header(ch_code=7), True), ((2, 24, 48000, 0), header(size_code=6), True),
            ((2, 17, 48000, 0), header(size_code=0), True), ((2, 17, 48000, 0), header(size_code=4), False),
            ((2, 16, 44100, 0), header(sr_code=9), True), ((2, 16, 655350, 0), header(sr_code=14, rate_field=65535), True),
            ((2, 16, 48000, 4096), header(), True), ((2, 16, 48000, 16), header(bs_code=6, n=16), True)]
    return out


def catalogue():
    """[(format, bytes, avail)]: every valid header whole, behind spare bytes, cut at every length, with every single
    bit flipped and against a stream whose largest block is one sample shorter; then the field cases."""
    cases = []
    for h in valid_headers():
        cases.append((BASE, h, len(h)))
        cases.append((BASE, h + b"\xff\xf8\x00", len(h) + 3))
        cases += [(BASE, h, avail) for avail in range(len(h))]
        for bit in range(8 * len(h)):
            x = bytearray(h)
            x[bit >> 3] ^= 0x80 >> (bit & 7)
            cases.append((BASE, bytes(x), len(h)))
        n = reference(BASE, h, len(h))[0]
        if n > 1:
            cases.append((BASE[:3] + (n - 1,), h, len(h)))
    cases += [(fmt, h, len(h)) for fmt, h, _ in field_cases()]
    return cases


# ---- the three builds ---------------------------------------------------------------------------------------

def build(tmp, name, compiler, extra):
    exe = tmp / name
    subprocess.run([*compiler, "-O1", "-g", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", str(exe)], check=True,
                   capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flac_header")
    return {"c99": build(tmp, "dump_c", ["gcc", "-std=gnu99"], []),
            "c++17": build(tmp, "dump_cxx", ["g++", "-std=c++17", "-x", "c++"], []),
            "sanitized": build(tmp, "dump_san", ["gcc", "-std=gnu99"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}


def run(exe, cases):
    words, fmt = [], None
    for f, data, avail in cases:
        if f != fmt:
            words.append("F %d %d %d %d" % f)
            fmt = f
        words.append("C %d %s" % (avail, bytes(data[:avail]).hex() or "-"))
    p = subprocess.run([exe], input="\n".join(words) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]              # (a sanitizer report ends the program with an error)
    assert p.stderr == ""
    out = []
    for line in p.stdout.splitlines():
        w = list(map(int, line.split()))
        out.append(tuple(w[1:]) if w[0] else None)
    assert len(out) == len(cases)
    return out


def test_three_builds_agree_with_each_other_and_with_the_format(builds):
    cases = catalogue()
    want = [reference(*c) for c in cases]
    assert sum(w is not None for w in want) >= 40 and sum(w is None for w in want) >= 200
    got = {name: run(exe, cases) for name, exe in builds.items()}
    for name in got:
        wrong = [(c, g, w) for c, g, w in zip(cases, got[name], want) if g != w]
        assert not wrong, (name, len(wrong), wrong[:5])
    assert got["c99"] == got["c++17"] == got["sanitized"]


def test_the_catalogue_holds_what_it_should():
    """The reference on the cases whose answer is known beforehand."""
    valid = valid_headers()
    assert all(reference(BASE, h, len(h)) is not None for h in valid) and len(valid) >= 40
    assert min(map(len, valid)) == 6 and max(map(len, valid)) == 16
    assert reference(BASE, header(bs_code=7, n=65535), 8) == (65535, 0, 8, 0)
    assert reference(BASE, header(bs_code=7, n=65536), 8) is None
    assert reference(BASE, header(number=(1 << 36) - 1, vbs=1), 12) == (4096, 1, 12, (1 << 36) - 1)
    assert reference(BASE, header(bs_code=6, n=256, sr_code=12, rate_field=48, number=0x80), 9) == (256, 0, 9, 0x80)
    for fmt, h, ok in field_cases():
        assert (reference(fmt, h, len(h)) is not None) == ok, (fmt, h.hex())
    h = header()
    assert all(reference(BASE, h, avail) is None for avail in range(len(h)))
    assert reference(BASE[:3] + (4095,), h, len(h)) is None and reference(BASE[:3] + (4096,), h, len(h)) is not None
