"""Writing seek tables without a GPU: flake_amd_write_seektable against struct.pack and back through the reader, with
every refusal; the recorder (flake_amd/host/seekpoints.h) through a stand-alone program (tools/seekpoints_dump.c) built
with -fsanitize=address,undefined, against the rule restated in seekpoints_rule.py; flake_amd_seekpoints_of_frames on a
fixed-block and a variable-block-size stream made by flacgen.py; and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import flacgen
import flake_amd
from seekpoints_rule import PLACEHOLDER, as_tuples, rule, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "seekpoints_dump.c")
V = flake_amd
POINTS = [(0, 0, 4096), (40960, 51234, 4096), (81920, 100001, 16), (2 ** 36 - 4096, 2 ** 40 + 3, 65535)]
MAX_POINTS = 932067                                          # (2^24 - 1) // 18


# ---- the writer ----

def test_writer_bytes_and_round_trip():
    for pts, ph in ((POINTS, 0), (POINTS, 3), (POINTS[:1], 1), ([], 2), ([], 0)):
        data = V.write_seektable(pts, ph)
        assert data == table(list(pts) + [PLACEHOLDER] * ph)
        back, n = V.read_seektable(data)
        assert n == len(pts) and as_tuples(back) == list(pts)
    back, _ = V.read_seektable(table(POINTS))
    assert V.write_seektable(back) == table(POINTS)                      # the reader's own array goes straight back in


def test_writer_refusals_leave_the_buffer_untouched():
    lib = V.load_host_library()
    pts = np.zeros(len(POINTS), V.SEEK_POINT_DTYPE)
    for i, p in enumerate(POINTS):
        pts[i] = (*p, 0)
    buf = np.full(18 * 8, 0xA5, np.uint8)

    def refused(points, n, ph, block=buf, cap=None):
        r = lib.flake_amd_write_seektable(points.ctypes.data if points is not None else None, n, ph,
                                          block.ctypes.data if block is not None else None, buf.size if cap is None else cap)
        return r == -1 and bool((buf == 0xA5).all())

    assert lib.flake_amd_write_seektable(pts.ctypes.data, 4, 2, buf.ctypes.data, buf.size) == 18 * 6       # it does write
    assert bytes(buf[:18 * 6]) == table(POINTS + [PLACEHOLDER] * 2)
    buf[:] = 0xA5
    assert refused(None, 1, 0) and refused(pts, 4, 0, block=None)        # a null pointer with a non-zero count
    assert refused(pts, -1, 0) and refused(pts, 4, -1)                   # a negative count
    swapped, equal, holder = pts.copy(), pts.copy(), pts.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    equal[2]["sample"] = equal[1]["sample"]
    holder[3]["sample"] = 2 ** 64 - 1
    assert refused(swapped, 4, 0) and refused(equal, 4, 0) and refused(holder, 4, 0)
    assert refused(pts, 4, 0, cap=18 * 4 - 1) and refused(pts, 4, 2, cap=18 * 5) and refused(pts, 0, 1, cap=17)
    assert refused(pts, 4, MAX_POINTS - 3, cap=2 ** 40) and refused(pts, 0, MAX_POINTS + 1, cap=2 ** 40)
    with pytest.raises(ValueError):
        V.write_seektable([POINTS[1], POINTS[0]])


def test_writer_takes_the_largest_table_a_block_holds():
    data = V.write_seektable(POINTS, MAX_POINTS - len(POINTS))
    assert len(data) == 18 * MAX_POINTS < 2 ** 24 and data[:18 * 4] == table(POINTS)
    assert data[18 * 4:] == table([PLACEHOLDER]) * (MAX_POINTS - 4)
    assert V.read_seektable(data, cap=4)[1] == 4


# ---- the recorder, sanitized ----

@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seekrec") / "seekpoints_san"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flake_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", str(exe)], check=True, capture_output=True, timeout=120)
    return str(exe)


def record(exe, spacing, ops):
    """ops: (samples, bytes, first_frame) for a block, "save", "restore".  (points, (samples, bytes, count))."""
    words = [spacing, len(ops)]
    for op in ops:
        words += [0, *op] if isinstance(op, tuple) else [1 if op == "save" else 2]
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    rows = [line.split() for line in p.stdout.split("\n") if line]
    return [tuple(map(int, r[1:])) for r in rows if r[0] == "P"], tuple(map(int, rows[-1][1:]))


def blocks_of(sizes, seed=0):
    """Blocks of these samples with made-up byte counts and first-frame sizes (a block may be several frames)."""
    return [(n, 11 + (7 * i + seed) % 23 + n // 3, n if i % 3 else max(1, n // 2)) for i, n in enumerate(sizes)]


def held_to_the_rule(exe, spacing, blocks):
    pts, counters = record(exe, spacing, blocks)
    want = rule(blocks, spacing)
    assert pts == want
    assert counters == (sum(b[0] for b in blocks), sum(b[1] for b in blocks), len(want))
    return pts


@pytest.mark.parametrize("spacing", [1, 64, 65, 200, 2 ** 40])
def test_blocks_of_64_with_a_tail(sanitized, spacing):
    pts = held_to_the_rule(sanitized, spacing, blocks_of([64] * 30 + [13]))
    assert pts[0][:2] == (0, 0)                               # the first block always gets one
    assert len(pts) == {1: 31, 64: 31, 65: 30, 200: 10, 2 ** 40: 1}[spacing]


def test_blocks_of_one_sample(sanitized):
    for spacing in (1, 3, 1000):
        pts = held_to_the_rule(sanitized, spacing, blocks_of([1] * 300, seed=5))
        assert [p[0] for p in pts] == list(range(0, 300, spacing))


def test_a_block_longer_than_several_spacings(sanitized):
    pts = held_to_the_rule(sanitized, 100, blocks_of([64, 1000, 64, 36, 64], seed=2))
    assert [p[0] for p in pts] == [0, 64, 1064, 1164]          # one point for the long block, then the target behind it
    held_to_the_rule(sanitized, 1, blocks_of([65535] * 40))    # spacing 1 with long blocks: no spinning
    assert record(sanitized, 0, blocks_of([64] * 5))[0] == []  # spacing 0 is off


def test_save_and_restore(sanitized):
    head, three, tail = blocks_of([64] * 7), blocks_of([64, 64, 13], seed=9), blocks_of([64] * 4, seed=3)
    for spacing in (64, 100, 150):
        pts, counters = record(sanitized, spacing, head + ["save"] + three + ["restore"] + three + tail)
        assert pts == rule(head + three + tail, spacing)
        assert counters[0] == 64 * 11 + 141
        # restored and left there: what the three blocks added is gone
        pts, counters = record(sanitized, spacing, head + ["save"] + three + ["restore"])
        assert pts == rule(head, spacing) and counters[:2] == (64 * 7, sum(b[1] for b in head))


def test_counters_past_32_bits(sanitized):
    big = [(2 ** 31, 2 ** 33 + 5, 4096)] * 5 + [(4096, 9000, 4096)] * 3
    pts = held_to_the_rule(sanitized, 2 ** 32, big)
    assert [p[0] for p in pts] == [0, 2 ** 32, 2 ** 33] and pts[2][1] == 4 * (2 ** 33 + 5)
    held_to_the_rule(sanitized, 4096, big)
    held_to_the_rule(sanitized, 2 ** 63 + 1, big + [(2 ** 63, 1, 1), (2 ** 62, 1, 1)])     # the next target does not fit 64 bits


# ---- flake_amd_seekpoints_of_frames ----

def made_stream(sizes, vbs):
    """A mono 16-bit stream of frames of these sizes (flacgen), its STREAMINFO and its frames' byte sizes."""
    sub = [dict(kind="fixed", order=2, porder=0)]
    frames, first = [], 0
    for i, n in enumerate(sizes):
        frames.append(flacgen.frame(flacgen.test_signal(n, 1, 16, seed=i), first if vbs else i, 16, 44100, sub, vbs=vbs))
        first += n
    si = V.HostStreaminfo(min_block_size=min(sizes) if vbs else sizes[0], max_block_size=max(sizes), sample_rate=44100,
                          channels=1, bits_per_sample=16, samples=sum(sizes))
    return si, b"".join(frames), [len(f) for f in frames]


@pytest.mark.parametrize("vbs, sizes", [(False, [192] * 9 + [50]), (True, [256, 100, 512, 192, 1000, 16, 16, 700, 31])])
def test_seekpoints_of_frames(vbs, sizes):
    si, stream, lens = made_stream(sizes, vbs)
    found, used = V.index_frames(si, stream)
    assert list(found) == lens and used == len(stream)
    for spacing in (1, 192, 200, 500, 10 ** 9):
        pts = V.seekpoints_of_frames(si, stream, found, spacing)
        assert as_tuples(pts) == rule([(n, b, n) for n, b in zip(sizes, lens)], spacing), spacing
    # a cap below the count: the count is still the whole, as with the reader
    lib = V.load_host_library()
    st, fs = np.frombuffer(stream, np.uint8), np.ascontiguousarray(found, np.int32)
    two = np.zeros(2, V.SEEK_POINT_DTYPE)
    n = lib.flake_amd_seekpoints_of_frames(si, st.ctypes.data, st.size, fs.ctypes.data, len(fs), 1, two.ctypes.data, 2)
    assert n == len(sizes) and as_tuples(two) == [(0, 0, sizes[0]), (sizes[0], lens[0], sizes[1])]
    # bad arguments
    assert lib.flake_amd_seekpoints_of_frames(si, st.ctypes.data, st.size, fs.ctypes.data, len(fs), 0, None, 0) == -1
    assert lib.flake_amd_seekpoints_of_frames(si, st.ctypes.data, st.size - 1, fs.ctypes.data, len(fs), 64, None, 0) == -1
    assert lib.flake_amd_seekpoints_of_frames(None, st.ctypes.data, st.size, fs.ctypes.data, len(fs), 64, None, 0) == -1
    assert lib.flake_amd_seekpoints_of_frames(si, st.ctypes.data, st.size, fs.ctypes.data, len(fs), 64, None, 1) == -1


@pytest.mark.parametrize("vbs, sizes", [(False, [192] * 4), (True, [256, 100, 512])])
def test_one_broken_header_byte_is_refused(vbs, sizes):
    si, stream, lens = made_stream(sizes, vbs)
    assert len(V.seekpoints_of_frames(si, stream, lens, 64)) > 0
    for frame in range(len(sizes)):
        for byte in (0, 1, 2, 3, 4):                          # sync, codes, the number: the CRC-8 no longer holds
            bad = bytearray(stream)
            bad[sum(lens[:frame]) + byte] ^= 0x10
            with pytest.raises(ValueError):
                V.seekpoints_of_frames(si, bytes(bad), lens, 64)


# ---- the command line's refusals ----

@pytest.mark.parametrize("args", [("--synth", 2, "--seekpoints", 0, "out.flac"),
                                  ("--set", "outdir", "--seekpoints", 0, "a.wav"),
                                  ("--recode", "--set", "outdir", "--seekpoints", 0, "a.flac"),
                                  ("--decode", "--seekpoints", 256, "a.flac", "a.wav"),
                                  ("--decode", "--set", "outdir", "--seekpoints", 256, "a.flac"),
                                  ("--reseek", 256, "a.flac"),
                                  ("--reseek", 0, "--set", "outdir", "a.flac")])
def test_cli_refusals(tmp_path, args):
    p = subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), *map(str, args)], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert p.returncode == 2 and "usage" in p.stderr and "--seekpoints" in p.stderr
    assert os.listdir(tmp_path) == []                         # nothing was written
