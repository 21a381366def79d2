"""flake_amd_read_seektable and flake_amd_seek_lookup (flake_amd/host/seektable.h): blocks packed with struct -- placeholders,
unsorted points, a length of 17, a cap smaller than the block -- and lookups before the first point, at a point and behind
the last; through the library, and through a stand-alone program (tools/seektable_dump.c) built with
-fsanitize=address,undefined whose block and point table are exactly as large as asked.  Runs without a GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "seektable_dump.c")
PLACEHOLDER = (2 ** 64 - 1, 0, 0)
POINTS = [(0, 0, 4096), (40960, 51234, 4096), (81920, 100001, 4096), (2 ** 36 - 4096, 2 ** 40 + 3, 65535)]


def block(points):
    return b"".join(struct.pack(">QQH", *p) for p in points)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = tmp_path_factory.mktemp("seek") / "seektable_san"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "flake_amd", "host"), "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", str(exe)], check=True, capture_output=True, timeout=120)
    return str(exe)


def program(exe, data, cap, lookups=()):
    words = [len(data), cap, len(lookups), *data, *lookups]
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    rows = [line.split() for line in p.stdout.split("\n") if line]
    return (int(rows[0][1]), [tuple(map(int, r[1:])) for r in rows if r[0] == "P"], [int(r[1]) for r in rows if r[0] == "L"])


def test_points_and_placeholders():
    pts, n = flake_amd.read_seektable(block(POINTS + [PLACEHOLDER, PLACEHOLDER]))
    assert n == 4 and [tuple(int(v) for v in (p["sample"], p["offset"], p["frame_samples"])) for p in pts] == POINTS
    pts, n = flake_amd.read_seektable(block([PLACEHOLDER] + POINTS[:2] + [PLACEHOLDER] + POINTS[2:]))      # anywhere
    assert n == 4 and list(pts["sample"]) == [p[0] for p in POINTS]
    assert flake_amd.read_seektable(b"")[1] == 0 and flake_amd.read_seektable(block([PLACEHOLDER]))[1] == 0


def test_refusals():
    for bad in (block(POINTS)[:17], block(POINTS)[:-1], block(POINTS) + b"\0",
                block([POINTS[1], POINTS[0]]), block([POINTS[0], POINTS[0]]), block(POINTS + [POINTS[1]])):
        with pytest.raises(ValueError):
            flake_amd.read_seektable(bad)
    lib = flake_amd.load_host_library()
    assert lib.flake_amd_read_seektable(None, 18, None, 0) == -1
    buf = np.frombuffer(block(POINTS), np.uint8)
    assert lib.flake_amd_read_seektable(buf.ctypes.data, buf.size, None, 1) == -1
    assert lib.flake_amd_read_seektable(buf.ctypes.data, buf.size, None, -1) == -1
    assert lib.flake_amd_read_seektable(buf.ctypes.data, buf.size, None, 0) == 4          # counting alone


def test_cap_smaller_than_the_block():
    pts, n = flake_amd.read_seektable(block(POINTS), cap=2)
    assert n == 4 and len(pts) == 2 and list(pts["offset"]) == [0, 51234]


def test_lookup():
    pts, _ = flake_amd.read_seektable(block(POINTS[1:]))
    assert flake_amd.seek_lookup(pts, 0) == -1 and flake_amd.seek_lookup(pts, 40959) == -1      # before the first point
    assert flake_amd.seek_lookup(pts, 40960) == 0 and flake_amd.seek_lookup(pts, 81919) == 0    # at a point, behind it
    assert flake_amd.seek_lookup(pts, 81920) == 1
    assert flake_amd.seek_lookup(pts, 2 ** 36) == 2 and flake_amd.seek_lookup(pts, 2 ** 64 - 1) == 2   # behind the last
    assert flake_amd.seek_lookup(pts[:0], 5) == -1
    assert flake_amd.load_host_library().flake_amd_seek_lookup(None, 3, 5) == -1


def test_the_same_through_a_sanitized_program(sanitized):
    looks = [0, 40959, 40960, 81919, 81920, 2 ** 36, 2 ** 64 - 1]
    data = block(POINTS[1:] + [PLACEHOLDER])
    n, pts, got = program(sanitized, data, 3, looks)
    assert n == 3 and pts == POINTS[1:] and got == [-1, -1, 0, 0, 1, 2, 2]
    n, pts, got = program(sanitized, data, 1, looks)                     # one point stored: the table has one entry
    assert n == 3 and pts == POINTS[1:2] and got == [-1, -1, 0, 0, 0, 0, 0]
    n, pts, got = program(sanitized, data, 0, looks[:2])
    assert n == 3 and pts == [] and got == [-1, -1]
    assert program(sanitized, data[:17], 4)[0] == -1
    assert program(sanitized, block([POINTS[2], POINTS[1]]), 4)[0] == -1
    assert program(sanitized, b"", 4, [7]) == (0, [], [-1])
