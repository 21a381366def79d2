"""The window planner (flake_amd/host/decode_window_plan.h) on its own: which frames of a run cover a window of samples,
the skip and take the device is given, and how the selected frames are cut into batches.  The planner makes no HIP call,
so a host program (tools/decode_window_plan_dump.c) runs it here without a GPU and prints its tables -- once built plain,
once with -fsanitize=address,undefined, every array and every run's bytes exactly as large as promised.  The runs are
header tables written out by hand below, and so are the expected tables."""
import os
import subprocess

import pytest

import flacgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "decode_window_plan_dump.c")
FMT = (1, 16, 44100, 0)          # mono, 16 bits, 44.1 kHz, no block-size limit
OK, EMPTY, FAILED = 0, 1, -1


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, SRC, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wplan"), "dump", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("wplan_san"), "dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def frame(number, n, vbs=False, broken=False):
    """A frame as far as the planner reads it: a mono 16-bit 44.1 kHz header (block size as an 8-bit field) and three
    bytes that stand for the rest."""
    h = bytes([0xFF, 0xF8 | int(vbs), 0x69, 0x08]) + flacgen.utf8(number) + bytes([n - 1])
    c = flacgen.crc8(h)
    return h + bytes([c ^ (0x55 if broken else 0)]) + b"\0\0\0"


# A: a fixed-block stream, ten frames numbered 0 .. 9, 192 samples each, the last 100 (1828 samples); 10 bytes a frame
A = [frame(k, 192) for k in range(9)] + [frame(9, 100)]
# V: a variable-block-size stream: sizes 100, 50, 200, 16, 134 from sample 1000 on (it ends at 1500); 11 bytes a frame
V = [frame(s, n, vbs=True) for s, n in ((1000, 100), (1100, 50), (1150, 200), (1350, 16), (1366, 134))]


def with_broken(frames, k, **kw):
    out = list(frames)
    out[k] = frame(k, 192, broken=True, **kw)
    return out


def run(exe, windows, max_batch=16):
    """windows: [(frames, fixed block size, first sample, count)].  Returns (W rows, batches [(B row, [S rows])], E row)."""
    words = [*FMT, max_batch, len(windows)]
    for frames, fixed, first, count in windows:
        words += [len(frames), fixed, first, count, *[len(f) for f in frames], *b"".join(frames)]
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    sel, batches, end = [], [], None
    for line in p.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        row = tuple(map(int, w[1:]))
        if w[0] == "W":
            sel.append(row)
        elif w[0] == "B":
            batches.append((row, []))
        elif w[0] == "S":
            batches[-1][1].append(row)
        elif w[0] == "E":
            end = row
    return sel, batches, end


NOTHING = (EMPTY, 0, 0, 0, 0, -1, 0, 0, 0, 0)
# (run, fixed block size, first sample, count) -> status frame0 nframes byte0 nbytes number variable skip take deliver
SELECT = [
    ((A, 192, 200, 5), (OK, 1, 1, 10, 10, 1, 0, 8, 5, 5)),                  # inside one frame
    ((A, 192, 190, 196), (OK, 0, 3, 0, 30, 0, 0, 190, 196, 196)),           # across three frames
    ((A, 192, 384, 7), (OK, 2, 1, 20, 10, 2, 0, 0, 7, 7)),                  # from a frame's first sample
    ((A, 192, 197, 187), (OK, 1, 1, 10, 10, 1, 0, 5, 187, 187)),            # to a frame's last sample
    ((A, 192, 577, 1), (OK, 3, 1, 30, 10, 3, 0, 1, 1, 1)),                  # one sample
    ((A, 192, 0, 1828), (OK, 0, 10, 0, 100, 0, 0, 0, 1828, 1828)),          # the whole run
    ((A, 192, 192, 192), (OK, 1, 1, 10, 10, 1, 0, 0, 192, 192)),            # exactly one frame
    ((A, 192, 5, 0), NOTHING),                                             # count 0
    ((A, 192, 1828, 4), NOTHING),                                          # begins at the run's end
    ((A, 192, 5000, 4), NOTHING),                                          # ... and behind it
    ((A, 192, 1800, 100), (OK, 9, 1, 90, 10, 9, 0, 72, 100, 28)),          # ends behind the run: cut there
    ((A, 0, 200, 5), (OK, 1, 1, 10, 10, 1, 0, 8, 5, 5)),                    # no STREAMINFO size: the first frame's
    # a run that starts mid-stream: frames 5 .. 9
    ((A[5:], 192, 1000, 300), (OK, 0, 2, 0, 20, 5, 0, 40, 300, 300)),
    ((A[5:], 0, 1000, 300), (OK, 0, 2, 0, 20, 5, 0, 40, 300, 300)),
    ((A[5:], 192, 900, 100), NOTHING),                                     # begins before the run's first frame
    ((A[5:], 192, 959, 2), NOTHING),
    # a run that is only the short last frame: its size is not the stream's
    ((A[9:], 192, 1730, 50), (OK, 0, 1, 0, 10, 9, 0, 2, 50, 50)),
    ((A[9:], 192, 1730, 500), (OK, 0, 1, 0, 10, 9, 0, 2, 500, 98)),
    # the variable stream: the numbers are samples
    ((V, 0, 1120, 240), (OK, 1, 3, 11, 33, 1100, 1, 20, 240, 240)),
    ((V, 4096, 1000, 1), (OK, 0, 1, 0, 11, 1000, 1, 0, 1, 1)),
    ((V, 0, 1365, 1000), (OK, 3, 2, 33, 22, 1350, 1, 15, 1000, 135)),
    ((V, 0, 999, 10), NOTHING),
    ((V, 0, 1500, 10), NOTHING),
    # a broken header: frame 8 is not probed for a window in frame 1 (the probes are 5, 2, 1, then 5, 3, 2) ...
    ((with_broken(A, 8), 192, 200, 5), (OK, 1, 1, 10, 10, 1, 0, 8, 5, 5)),
    # ... and is for a window in frame 8 (5, 7, 8)
    ((with_broken(A, 8), 192, 1600, 10), (FAILED, 0, 0, 0, 0, -1, 0, 0, 0, 0)),
    ((with_broken(A, 0), 192, 200, 5), (FAILED, 0, 0, 0, 0, -1, 0, 0, 0, 0)),       # the run's first header is always read
    ((with_broken(V, 2, vbs=True), 0, 1000, 10), (FAILED, 0, 0, 0, 0, -1, 0, 0, 0, 0)),
]


def test_selection(plain):
    sel, batches, end = run(plain, [w for w, _ in SELECT])
    for (w, want), got in zip(SELECT, sel):
        assert got == want, (w[1:], got, want)
    assert len(sel) == len(SELECT)
    assert end == tuple(want[0] for _, want in SELECT)


# three windows for the cuts: frames 0 .. 2 of A, frame 1 of A, frames 1 .. 3 of V
CUTS = [(A, 192, 190, 196), (A, 192, 200, 5), (V, 0, 1120, 240)]
# max_batch -> [(nframes nsegs nbytes), [first number variable skip take win frame0 last]]
BATCHES = {
    16: [((7, 3, 73), [(0, 0, 0, 190, 196, 0, 0, 1), (3, 1, 0, 8, 5, 1, 1, 1), (4, 1100, 1, 20, 240, 2, 1, 1)])],
    # a cut behind frame 1 of window 0: 384 samples lie before it, 190 of them dropped, 194 delivered, 2 left to take
    2: [((2, 1, 20), [(0, 0, 0, 190, 196, 0, 0, 0)]),
        ((2, 2, 20), [(0, 2, 0, 0, 2, 0, 2, 1), (1, 1, 0, 8, 5, 1, 1, 1)]),
        ((2, 1, 22), [(0, 1100, 1, 20, 240, 2, 1, 0)]),                  # 250 samples, 20 dropped: 10 left to take
        ((1, 1, 11), [(0, 1350, 1, 0, 10, 2, 3, 1)])],
    1: [((1, 1, 10), [(0, 0, 0, 190, 196, 0, 0, 0)]),                    # 192 samples, 190 dropped: 2 delivered
        ((1, 1, 10), [(0, 1, 0, 0, 194, 0, 1, 0)]),
        ((1, 1, 10), [(0, 2, 0, 0, 2, 0, 2, 1)]),
        ((1, 1, 10), [(0, 1, 0, 8, 5, 1, 1, 1)]),
        ((1, 1, 11), [(0, 1100, 1, 20, 240, 2, 1, 0)]),                  # 50 samples, 20 dropped: 30 delivered
        ((1, 1, 11), [(0, 1150, 1, 0, 210, 2, 2, 0)]),                   # 200 more
        ((1, 1, 11), [(0, 1350, 1, 0, 10, 2, 3, 1)])],
}


@pytest.mark.parametrize("max_batch", sorted(BATCHES))
def test_batch_cuts(plain, max_batch):
    sel, batches, end = run(plain, CUTS, max_batch)
    assert batches == BATCHES[max_batch]
    assert end == (OK, OK, OK)


def test_a_skip_larger_than_the_first_part(plain):
    """A stream whose numbers jump: the window begins behind the frame the search lands on, and the skip outlives a cut."""
    J = [frame(0, 192), frame(1, 192), frame(5, 192), frame(6, 192)]
    # sample 500 lies in no frame (1 ends at 384, 5 begins at 960): the search lands on frame 1, 308 samples before it
    sel, batches, end = run(plain, [(J, 192, 500, 600)], 1)
    assert sel == [(OK, 1, 2, 10, 20, 1, 0, 308, 600, 600)]
    # the cut behind frame 1: by the numbers 768 samples lie before frame 5, so the skip is used up there
    assert batches == [((1, 1, 10), [(0, 1, 0, 308, 600, 0, 1, 0)]), ((1, 1, 10), [(0, 5, 0, 0, 140, 0, 2, 1)])]


def test_a_broken_header_at_a_cut_fails_the_window(plain):
    """Frame 3 is broken and no probe of the selection reads it (5, 2, 1, then 5, 7, 8, 9): the cut behind frame 2 does."""
    B = with_broken(A, 3)
    sel, batches, end = run(plain, [(B, 192, 200, 1500), (A, 192, 200, 5)], 2)
    assert sel == [(OK, 1, 8, 10, 80, 1, 0, 8, 1500, 1500), (OK, 1, 1, 10, 10, 1, 0, 8, 5, 5)]
    assert batches == [((1, 1, 10), [(0, 1, 0, 8, 5, 1, 1, 1)])]           # the other window is planned as ever
    assert end == (FAILED, OK)
    # with room for the whole sub-run nothing is cut and the device is the one to find the header
    sel, batches, end = run(plain, [(B, 192, 200, 1500)], 16)
    assert end == (OK,) and batches == [((8, 1, 80), [(0, 1, 0, 8, 1500, 0, 1, 1)])]


def test_every_case_again_under_the_sanitizers(plain, sanitized):
    """The same program with -fsanitize=address,undefined: it ends cleanly (a report aborts it) with the same output."""
    calls = [([w for w, _ in SELECT], 16), (CUTS, 1), (CUTS, 2), (CUTS, 16), ([(with_broken(A, 3), 192, 200, 1500)], 2),
             ([(A[:1], 192, 0, 5), ([], 192, 0, 5), (A, 192, 0, 1828)], 3)]
    for windows, mb in calls:
        assert run(sanitized, windows, mb) == run(plain, windows, mb)
