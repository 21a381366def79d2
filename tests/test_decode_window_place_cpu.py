"""The window placement (flake_amd/host/decode_window_place.h) on its own: where the samples of each window of a
flake_amd_decode_set_windows call land in the output, batch by batch, and what a failed window costs.  The header makes
no HIP call, so a host program (tools/decode_window_place_dump.c) runs it here without a GPU and prints its tables --
once built plain, once with -fsanitize=address,undefined, every table exactly as large as promised.  The batches are
written out by hand below, as the planner and the device would leave them, and so are the expected tables: from the rule
at the top of the header, not from running the code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "decode_window_place_dump.c")
OK, EMPTY, FAILED = 0, 1, -1         # a window's selection (FA_DW_*)
HEADER, CRC = 1, 4                   # a window's status: the planner's failure, and a frame's as the device reports it


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, SRC, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wplace"), "dump", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wplace_san"), "dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def seg(win, last, samples, failed=-1, status=0):
    return (win, last, samples, failed, status)


def run(exe, windows, batches, rows=True, end_changes=()):
    """windows: [(selection status, count)]; batches: [[segment]] or [(changes, [segment])] with changes [(window, status)].
    Returns (batches [(base, [(target, row, col)])], windows [(at, samples, status)], total)."""
    words = [int(rows), len(windows), *[v for w in windows for v in w], len(batches)]
    for b in batches:
        ch, segs = b if isinstance(b, tuple) else ((), b)
        words += [len(ch), *[v for c in ch for v in c], len(segs), *[v for s in segs for v in s]]
    words += [len(end_changes), *[v for c in end_changes for v in c]]
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    out, wins, total = [], [], None
    for line in p.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        row = tuple(map(int, w[1:]))
        if w[0] == "B":
            out.append((row[0], []))
        elif w[0] == "S":
            out[-1][1].append(row)
        elif w[0] == "W":
            wins.append(row)
        elif w[0] == "T":
            total = row[0]
    return out, wins, total


# three windows of 100, 200 and 50 samples; the middle one is cut: 120 samples in its first part
THREE = [(OK, 100), (OK, 200), (OK, 50)]


def test_three_good_windows_in_two_batches(plain):
    got = run(plain, THREE, [[seg(0, 1, 100), seg(1, 0, 120)], [seg(1, 1, 80), seg(2, 1, 50)]])
    # the second batch is written from 220 on; the middle window's second part goes to row 1 at column 120
    assert got == ([(0, [(0, 0, 0), (100, 1, 0)]), (220, [(220, 1, 120), (300, 2, 0)])],
                   [(0, 100, 0), (100, 200, 0), (300, 50, 0)], 350)


def test_every_segment_its_own_batch(plain):
    got = run(plain, THREE, [[seg(0, 1, 100)], [seg(1, 0, 120)], [seg(1, 1, 80)], [seg(2, 1, 50)]])
    assert got == ([(0, [(0, 0, 0)]), (100, [(100, 1, 0)]), (220, [(220, 1, 120)]), (300, [(300, 2, 0)])],
                   [(0, 100, 0), (100, 200, 0), (300, 50, 0)], 350)


def test_the_middle_window_fails_on_the_device_in_its_second_segment(plain):
    """Its first segment delivered 120 samples to 100 .. 220.  The second fails: the window's count becomes -1, it keeps
    200 samples of room from 100 on, so the next window goes to 300 although the device wrote it from 220 on, and the
    third segment, sent when the failure is known, has row -1."""
    got = run(plain, THREE, [[seg(0, 1, 100), seg(1, 0, 120)], [seg(1, 0, 50, failed=0, status=CRC)],
                             [seg(1, 1, 30), seg(2, 1, 50)]])
    assert got == ([(0, [(0, 0, 0), (100, 1, 0)]), (220, [(-1, 1, 120)]), (220, [(-1, -1, 120), (300, 2, 0)])],
                   [(0, 100, 0), (100, -1, CRC), (300, 50, 0)], 150)
    # the same in two batches: the failing segment is the window's last, and the next window's target moves with it
    got = run(plain, THREE, [[seg(0, 1, 100), seg(1, 0, 120)], [seg(1, 1, 80, failed=1, status=CRC), seg(2, 1, 50)]])
    assert got == ([(0, [(0, 0, 0), (100, 1, 0)]), (220, [(-1, 1, 120), (300, 2, 0)])],
                   [(0, 100, 0), (100, -1, CRC), (300, 50, 0)], 150)


def seven(status):
    """Windows 1, 3 and 5 are good (20, 40, 60 samples); 0, 2, 4 and 6 have `status` and counts 10, 30, 50, 70: before the
    first batch's first window, between two windows of one batch, between two batches and after the last."""
    return [(status, 10), (OK, 20), (status, 30), (OK, 40), (status, 50), (OK, 60), (status, 70)]


SEVEN_BATCHES = [[seg(1, 1, 20), seg(3, 1, 40)], [seg(5, 1, 60)]]


def test_windows_that_failed_in_the_planner_keep_their_room(plain):
    got = run(plain, seven(FAILED), SEVEN_BATCHES)
    # 0 .. 10 is window 0's room, 30 .. 60 window 2's, 100 .. 150 window 4's, and window 6 begins at 210
    assert got == ([(10, [(10, 1, 0), (60, 3, 0)]), (150, [(150, 5, 0)])],
                   [(0, -1, HEADER), (10, 20, 0), (30, -1, HEADER), (60, 40, 0), (100, -1, HEADER), (150, 60, 0),
                    (210, -1, HEADER)], 120)


def test_windows_that_select_nothing_take_no_room(plain):
    got = run(plain, seven(EMPTY), SEVEN_BATCHES)
    assert got == ([(0, [(0, 1, 0), (20, 3, 0)]), (60, [(60, 5, 0)])],
                   [(0, 0, 0), (0, 20, 0), (20, 0, 0), (20, 40, 0), (60, 0, 0), (60, 60, 0), (120, 0, 0)], 120)


def test_a_window_the_planner_fails_at_a_cut(plain):
    """Window 0 asked for 100 samples and delivered 60 in its first part; the planner then finds no header at the cut and
    plans none of the rest.  The window keeps 100 samples of room: the next one goes to 100."""
    got = run(plain, [(OK, 100), (OK, 30)], [[seg(0, 0, 60)], ([(0, FAILED)], [seg(1, 1, 30)])])
    assert got == ([(0, [(0, 0, 0)]), (100, [(100, 1, 0)])], [(0, -1, HEADER), (100, 30, 0)], 30)
    # ... and as the call's last window: nothing is left to plan, and the end settles it
    got = run(plain, [(OK, 30), (OK, 100)], [[seg(0, 1, 30), seg(1, 0, 60)]], end_changes=[(1, FAILED)])
    assert got == ([(0, [(0, 0, 0), (30, 1, 0)])], [(0, 30, 0), (30, -1, HEADER)], 30)


def test_no_windows_and_no_rows(plain):
    assert run(plain, [], []) == ([], [], 0)
    got = run(plain, THREE, [[seg(0, 1, 100), seg(1, 1, 200), seg(2, 1, 50)]], rows=False)
    assert got == ([(0, [(0, 0, 0), (100, 0, 0), (300, 0, 0)])], [(0, 100, 0), (100, 200, 0), (300, 50, 0)], 350)


def test_every_case_again_under_the_sanitizers(plain, sanitized):
    """The same program with -fsanitize=address,undefined: it ends cleanly (a report aborts it) with the same output."""
    calls = [(THREE, [[seg(0, 1, 100), seg(1, 0, 120)], [seg(1, 1, 80), seg(2, 1, 50)]], {}),
             (THREE, [[seg(0, 1, 100)], [seg(1, 0, 120)], [seg(1, 1, 80)], [seg(2, 1, 50)]], {}),
             (THREE, [[seg(0, 1, 100), seg(1, 0, 120)], [seg(1, 0, 50, failed=0, status=CRC)], [seg(1, 1, 30), seg(2, 1, 50)]], {}),
             (seven(FAILED), SEVEN_BATCHES, {}), (seven(EMPTY), SEVEN_BATCHES, {}),
             ([(OK, 100), (OK, 30)], [[seg(0, 0, 60)], ([(0, FAILED)], [seg(1, 1, 30)])], {}),
             ([(OK, 30), (OK, 100)], [[seg(0, 1, 30), seg(1, 0, 60)]], dict(end_changes=[(1, FAILED)])),
             ([], [], {}), (THREE, [[seg(0, 1, 100), seg(1, 1, 200), seg(2, 1, 50)]], dict(rows=False))]
    for windows, batches, kw in calls:
        assert run(sanitized, windows, batches, **kw) == run(plain, windows, batches, **kw)
