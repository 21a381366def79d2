"""The table-block layout (flake_amd/csrc/table_block.h) on its own: api.hip puts a call's small tables into one block
of device memory and one host image, and where each table lies in it is this header's answer.  A host program
(tools/table_block_dump.cpp) lays out the blocks of fhip_decode_frames_segments, in each of its modes, and of
fhip_index_frames for 0 .. 9 segments or ranges and 0 .. 3 streams, and prints every slot; the properties are checked
here.  Built with -fsanitize=address,undefined the program fills every slot to its last byte in a block of exactly the
layout's size, so a slot that reaches past the total, or into its neighbour, ends it with a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flake_amd", "csrc")
SRC = os.path.join(ROOT, "tools", "table_block_dump.cpp")


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", CSRC, SRC, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


def run(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    return p.stdout


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp("tblock"), "dump", []))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return run(build(tmp_path_factory.mktemp("tblock_san"), "dump_san",
                     ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def cases(text):
    """[(name, ns, nst, total, [(offset, bytes, element size)])], and the H line's numbers."""
    out, head = [], None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "C":
            out.append((w[1], int(w[2]), int(w[3]), int(w[4]), []))
        elif w[0] == "S":
            out[-1][4].append(tuple(map(int, w[1:])))
        elif w[0] == "H":
            head = tuple(map(int, w[1:]))
    return out, head


# the tables of each block as (element size, count): written out here, not read from the program
def segment_tables(ns, nst, md5, win, rows):
    return [(8, ns), (8, ns), (8, ns), (4, ns + 1), (4, ns), (4, ns), (4, nst + 1 if md5 else 0), (4, ns if md5 else 0),
            (8, ns if win else 0), (8, ns if win else 0), (8, ns if rows else 0), (4, ns if rows else 0)]


MODES = {"segments": (False, False, False), "md5": (True, False, False), "windows": (False, True, False),
         "rows": (False, True, True)}
FCAPS = [0, 1, 2, 7, 65536, 65539]


def test_every_block_is_there(plain):
    got, _ = cases(plain)
    names = [(name, ns, nst) for name, ns, nst, _, _ in got]
    want = []
    for ns in range(10):
        want += [(m, ns, nst) for nst in range(4) for m in MODES]
        want += [("index", ns, fcap) for fcap in FCAPS]
    assert names == want


def test_slots_are_disjoint_aligned_in_order_and_inside_the_total(plain):
    got, _ = cases(plain)
    for name, ns, nst, total, slots in got:
        tables = ([(8, ns + 1), (8, ns), (4, ns), (4, ns), (4, nst)] if name == "index"
                  else segment_tables(ns, nst, *MODES[name]))
        assert len(slots) == len(tables)
        end = 0
        for (off, nbytes, elem), (want_elem, count) in zip(slots, tables):
            where = (name, ns, nst, off)
            assert elem == want_elem and nbytes == elem * count, where      # the size it was asked for
            assert off % 8 == 0 and off % elem == 0, where                  # aligned
            assert off >= end, where                                        # in order, and disjoint from the one before
            end = off + nbytes
        assert end <= total and total % 8 == 0 and total - end < 8, (name, ns, nst)    # inside the total, which wastes no word
        assert total <= sum(e * c for e, c in tables) + 7 * len(tables)     # padding only: less than a word per table


def test_an_empty_layout_and_an_empty_table(plain):
    got, _ = cases(plain)
    by = {(name, ns, nst): (total, slots) for name, ns, nst, total, slots in got}
    total, slots = by[("segments", 0, 0)]
    assert total == 8 and [s[1] for s in slots] == [0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0]      # seg_first [1] alone
    total, slots = by[("md5", 3, 2)]
    # 3 x 24 bytes, then 16 of 16, 12 of 16, 12 of 16, md5_first 12 of 16, md5_range 12 of 16: 152
    assert total == 152 and [s[0] for s in slots] == [0, 24, 48, 72, 88, 104, 120, 136, 152, 152, 152, 152]


def test_the_head_of_a_slot(plain):
    _, head = cases(plain)
    assert head == (24, 44, 24, 44)          # int32 [11] behind int64 [3]; its first 5 elements end at 24 + 20


def test_the_same_under_the_sanitizers(plain, sanitized):
    assert sanitized == plain
