"""The batch planner of a decode set (flake_amd/host/decode_set_plan.h) on its own: which frames of which run go into
which device batch, the segment tables, the numbering carried from batch to batch, K6's CSR and the refused calls.  The
planner makes no HIP call, so a host program (tools/decode_set_plan_dump.c) runs it here without a GPU and prints its
tables -- once built plain, once with -fsanitize=address,undefined, every array exactly as large as promised.  The
expected tables are written out by hand for the named cases and come from a model in Python for random calls."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "decode_set_plan_dump.c")

BAD_STREAM, BAD_COUNT, BAD_SIZE, FAILED_STREAM, NULL = -1, -2, -3, -4, -5


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, SRC, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plan"), "dump", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plan_san"), "dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, streams, max_batch, runs, sizes, nbytes=None, nstreams=None, null_sizes=False):
    """streams: [(started, variable, failed, next_number, samples per frame)]; runs: [(stream, frames)].  Returns the
    refusal code, or the batches as dicts."""
    nbytes = int(sum(sizes)) if nbytes is None else nbytes
    words = [len(streams) if nstreams is None else nstreams, max_batch, len(runs), -1 if null_sizes else len(sizes), nbytes]
    for s in streams:
        words += list(s)
    for r in runs:
        words += list(r)
    words += list(sizes)
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    out, batches = p.stdout.split("\n"), []
    if out[0].startswith("E"):
        return int(out[0].split()[1])
    for line in out:
        w = line.split()
        if not w:
            continue
        if w[0] == "B":
            batches.append(dict(zip(("frame0", "nframes", "nsegs", "byte0", "nbytes"), map(int, w[1:])), segs=[]))
        elif w[0] == "S":
            batches[-1]["segs"].append(tuple(map(int, w[1:])))      # first number variable stream run frame0 prev
        elif w[0] in "FMR":
            batches[-1][w[0]] = list(map(int, w[1:]))
        elif w[0] == "T":
            assert int(w[1]) == sum(f for _, f in runs)
    return batches


def model(streams, max_batch, runs, sizes):
    """The same plan, written the slow way: frame by frame."""
    st = [list(s) for s in streams]
    frames = [(r, s, k) for r, (s, n) in enumerate(runs) for k in range(n)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    out = []
    for f0 in range(0, len(frames), max_batch):
        part = frames[f0:f0 + max_batch]
        segs, last, planned = [], {}, {}
        for i, (r, s, k) in enumerate(part):
            if i == 0 or part[i - 1][0] != r:
                started, variable, failed, number, _ = st[s]
                if not started or failed:
                    num = -1
                elif not variable:
                    num = number + planned.get(s, 0)
                else:
                    num = number if s not in last else -1
                segs.append((i, num, int(bool(variable)), s, r, k, last.get(s, -1)))
                last[s] = len(segs) - 1
            planned[s] = planned.get(s, 0) + 1
        first = [g[0] for g in segs] + [len(part)]
        per = [[k for k, g in enumerate(segs) if g[3] == s] for s in range(len(st))]
        out.append(dict(frame0=f0, nframes=len(part), nsegs=len(segs), byte0=int(off[f0]), nbytes=int(off[f0 + len(part)] - off[f0]),
                        segs=segs, F=first, M=[0] + list(np.cumsum([len(p) for p in per])), R=[k for p in per for k in p]))
        for k, g in enumerate(segs):
            s, n = g[3], first[k + 1] - first[k]
            if st[s][0] and not st[s][2]:
                st[s][3] += n * st[s][4] if st[s][1] else n
    return out


FIXED = (1, 0, 0)
VAR = (1, 1, 0)


def test_runs_cut_at_batch_boundaries(plain):
    """Three fixed-block streams, runs of 3, 4 and 3 frames, batches of 4: run 1 is cut after one frame and its second
    part is numbered on from the first."""
    streams = [FIXED + (10, 64), FIXED + (0, 64), FIXED + (7, 64)]
    sizes = [10, 11, 12, 20, 21, 22, 23, 30, 31, 32]
    got = run(plain, streams, 4, [(0, 3), (1, 4), (2, 3)], sizes)
    assert [(b["frame0"], b["nframes"], b["byte0"], b["nbytes"]) for b in got] == [(0, 4, 0, 53), (4, 4, 53, 96), (8, 2, 149, 63)]
    assert got[0]["segs"] == [(0, 10, 0, 0, 0, 0, -1), (3, 0, 0, 1, 1, 0, -1)]
    assert got[1]["segs"] == [(0, 1, 0, 1, 1, 1, -1), (3, 7, 0, 2, 2, 0, -1)]
    assert got[2]["segs"] == [(0, 8, 0, 2, 2, 1, -1)]
    assert [b["F"] for b in got] == [[0, 3, 4], [0, 3, 4], [0, 2]]
    assert got[0]["M"] == [0, 1, 2, 2] and got[0]["R"] == [0, 1]
    assert got[1]["M"] == [0, 0, 1, 2] and got[1]["R"] == [0, 1]
    assert got == model(streams, 4, [(0, 3), (1, 4), (2, 3)], sizes)


def test_a_stream_with_several_runs_in_one_batch(plain):
    """Round-robin: fixed blocks are numbered on by the frames planned before; a variable-block-size stream's later
    segment waits for the samples of the earlier one (-1, linked through prev); K6 takes each stream's segments in order."""
    streams = [FIXED + (5, 64), VAR + (1000, 32)]
    runs = [(0, 2), (1, 2), (0, 1), (1, 3), (0, 2)]
    got = run(plain, streams, 16, runs, [9] * 10)
    assert len(got) == 1 and got[0]["nsegs"] == 5
    assert got[0]["segs"] == [(0, 5, 0, 0, 0, 0, -1), (2, 1000, 1, 1, 1, 0, -1), (4, 7, 0, 0, 2, 0, 0), (5, -1, 1, 1, 3, 0, 1),
                              (8, 8, 0, 0, 4, 0, 2)]
    assert got[0]["M"] == [0, 3, 5] and got[0]["R"] == [0, 2, 4, 1, 3]
    # the next call's first batch is numbered on: 5 frames of stream 0, 5 frames of 32 samples of stream 1
    again = run(plain, [FIXED + (10, 64), VAR + (1160, 32)], 16, [(1, 1), (0, 1)], [9, 9])
    assert again[0]["segs"] == [(0, 1160, 1, 1, 0, 0, -1), (1, 10, 0, 0, 1, 0, -1)]


def test_numbering_carries_across_batches_of_a_variable_stream(plain):
    streams = [VAR + (0, 48), FIXED + (3, 16)]
    got = run(plain, streams, 3, [(0, 7), (1, 2)], [5] * 9)
    assert [b["segs"] for b in got] == [[(0, 0, 1, 0, 0, 0, -1)], [(0, 144, 1, 0, 0, 3, -1)],
                                        [(0, 288, 1, 0, 0, 6, -1), (1, 3, 0, 1, 1, 0, -1)]]


def test_empty_runs_make_no_segment(plain):
    streams = [FIXED + (0, 16), FIXED + (0, 16), FIXED + (0, 16)]
    got = run(plain, streams, 8, [(0, 0), (1, 2), (2, 0), (2, 0), (0, 1), (1, 0)], [4, 4, 4])
    assert len(got) == 1 and got[0]["segs"] == [(0, 0, 0, 1, 1, 0, -1), (2, 0, 0, 0, 4, 0, -1)]
    assert got[0]["M"] == [0, 1, 2, 2] and got[0]["R"] == [1, 0]
    assert run(plain, streams, 8, [(0, 0), (1, 0)], []) == []
    assert run(plain, streams, 8, [], []) == []


def test_a_batch_of_exactly_the_limit(plain):
    streams = [FIXED + (0, 16), FIXED + (9, 16)]
    for total, want in ((8, [8]), (9, [8, 1]), (16, [8, 8]), (7, [7])):
        got = run(plain, streams, 8, [(0, 5), (1, total - 5)], [3] * total)
        assert [b["nframes"] for b in got] == want
        assert got == model(streams, 8, [(0, 5), (1, total - 5)], [3] * total)
    one = run(plain, streams, 1, [(0, 2), (1, 1)], [3, 4, 5])
    assert [b["segs"] for b in one] == [[(0, 0, 0, 0, 0, 0, -1)], [(0, 1, 0, 0, 0, 1, -1)], [(0, 9, 0, 1, 1, 0, -1)]]
    assert [(b["byte0"], b["nbytes"]) for b in one] == [(0, 3), (3, 4), (7, 5)]


def test_streams_not_started_or_failed_are_not_numbered(plain):
    """A stream whose first header could not be read stays unstarted (the set has failed it by then); a stream that
    fails during a call keeps its place in the later batches, unnumbered."""
    got = run(plain, [(0, 0, 0, 0, 16), FIXED + (4, 16)], 8, [(0, 2), (1, 2)], [3] * 4)
    assert got[0]["segs"] == [(0, -1, 0, 0, 0, 0, -1), (2, 4, 0, 1, 1, 0, -1)]
    # ... with the strategy bit its first frame shows, so that the device judges the frame and not the bit
    got = run(plain, [(0, 1, 0, 0, 16), FIXED + (4, 16)], 8, [(0, 2), (1, 2)], [3] * 4)
    assert got[0]["segs"] == [(0, -1, 1, 0, 0, 0, -1), (2, 4, 0, 1, 1, 0, -1)]


def test_refused_calls(plain):
    ok = [FIXED + (0, 16), FIXED + (0, 16)]
    assert run(plain, ok, 8, [(2, 1)], [5]) == BAD_STREAM
    assert run(plain, ok, 8, [(-1, 1)], [5]) == BAD_STREAM
    assert run(plain, ok, 8, [(0, -1)], []) == BAD_COUNT
    assert run(plain, ok, 8, [(0, 2)], [5, 6], nbytes=10) == BAD_SIZE          # the sizes run past the bytes
    assert run(plain, ok, 8, [(0, 2)], [5, 0], nbytes=10) == BAD_SIZE          # no frame is empty
    assert run(plain, ok, 8, [(0, 2)], [5, -3], nbytes=10) == BAD_SIZE
    assert run(plain, ok, 8, [(0, 2)], [5, 5], nbytes=10) != BAD_SIZE
    assert run(plain, [FIXED + (0, 16), (1, 0, 1, 0, 16)], 8, [(0, 1), (1, 1)], [5, 5]) == FAILED_STREAM
    assert run(plain, ok, 8, [(0, 1)], [5], nstreams=0) == BAD_COUNT
    assert run(plain, ok, 8, [(0, 1)], [5], null_sizes=True) == NULL


def test_fixed_block_size_rule_across_segments(tmp_path):
    """fa_ds_fixed_sizes: what the set holds a fixed-block stream to from segment to segment, where the device has no
    predecessor to compare with.  Each case is a list of segments (frames, first size, last size) -> the answers."""
    cases = [
        ([(3, 64, 64), (2, 64, 64), (4, 64, 40)], [0, 0, 0]),            # whole blocks, the short one at the very end
        ([(3, 64, 40), (1, 64, 64)], [0, -1]),                           # a frame behind a short one: cut or not, refused
        ([(3, 64, 64), (1, 40, 40), (1, 64, 64)], [0, 0, -1]),           # ... also when the short one is a segment alone
        ([(3, 64, 64), (1, 40, 40)], [0, 0]),                            # which by itself is the stream's last frame
        ([(2, 64, 64), (2, 48, 48)], [0, -1]),                           # another size in the middle
        ([(1, 40, 40), (1, 64, 64)], [0, -1]),                           # larger than the first
        ([(2, 64, 64), (2, 128, 128)], [0, -1]),
        ([(1, 64, 64), (1, 64, 64), (1, 64, 64)], [0, 0, 0]),
    ]
    body = []
    for segs, _ in cases:
        body.append("    { fa_ds_stream t; memset(&t, 0, sizeof t);\n")
        for nf, a, b in segs:
            body.append(f'      printf("%d\\n", fa_ds_fixed_sizes(&t, {nf}, {a}, {b}));\n')
        body.append("    }\n")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "decode_set_plan.h"\nint main(void)\n{\n' + "".join(body) +
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", HOST, str(src),
                    "-o", str(exe)], check=True, capture_output=True, timeout=120)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert out == [v for _, want in cases for v in want]


def random_calls():
    r = np.random.RandomState(20241019)
    out = []
    for _ in range(60):
        ns = int(r.randint(1, 9))
        streams = [(1, int(r.randint(0, 2)), 0, int(r.randint(0, 1000)), int(r.choice([16, 64, 4096]))) for _ in range(ns)]
        runs = [(int(r.randint(0, ns)), int(r.choice([0, 1, 2, 3, 7, 20]))) for _ in range(int(r.randint(0, 25)))]
        sizes = [int(x) for x in r.randint(1, 50, sum(f for _, f in runs))]
        out.append((streams, int(r.choice([1, 2, 3, 8, 16, 1024])), runs, sizes))
    return out


def test_random_calls_agree_with_the_model(plain):
    for streams, mb, runs, sizes in random_calls():
        assert run(plain, streams, mb, runs, sizes) == model(streams, mb, runs, sizes), (streams, mb, runs)


def test_every_case_again_under_the_sanitizers(plain, sanitized):
    """The same program with -fsanitize=address,undefined: it ends cleanly (a report aborts it) with the same output."""
    ok = [FIXED + (0, 16), FIXED + (0, 16)]
    calls = random_calls() + [
        ([FIXED + (10, 64), FIXED + (0, 64), FIXED + (7, 64)], 4, [(0, 3), (1, 4), (2, 3)], [10, 11, 12, 20, 21, 22, 23, 30, 31, 32]),
        ([FIXED + (5, 64), VAR + (1000, 32)], 16, [(0, 2), (1, 2), (0, 1), (1, 3), (0, 2)], [9] * 10),
        ([VAR + (0, 48), FIXED + (3, 16)], 3, [(0, 7), (1, 2)], [5] * 9),
        (ok + [FIXED + (0, 16)], 8, [(0, 0), (1, 2), (2, 0), (2, 0), (0, 1), (1, 0)], [4, 4, 4]),
        (ok, 8, [(0, 5), (1, 3)], [3] * 8), (ok, 8, [(0, 5), (1, 11)], [3] * 16), (ok, 1, [(0, 2), (1, 1)], [3, 4, 5]),
        (ok, 8, [], []), (ok, 8, [(2, 1)], [5]), (ok, 8, [(0, -1)], []), (ok, 8, [(0, 2)], [5, 0]),
    ]
    for streams, mb, runs, sizes in calls:
        assert run(sanitized, streams, mb, runs, sizes) == run(plain, streams, mb, runs, sizes)
    assert run(sanitized, ok, 8, [(0, 2)], [5, 6], nbytes=10) == BAD_SIZE
    assert run(sanitized, ok, 8, [(0, 1)], [5], null_sizes=True) == NULL
