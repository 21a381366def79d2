"""The planner of a recode set (flake_amd/host/recode_plan.h) on its own: how one decode batch's segments and the streams'
carries become the encoder's blocks and the new carries, as K9's piece tables.  It makes no HIP call, so a host program
(tools/recode_plan_dump.c) runs it here without a GPU and prints its tables -- once built plain, once with
-fsanitize=address,undefined, every array exactly as large as promised.  The expected tables are written out by hand for
the named cases; random calls are held against a model in Python that moves sample by sample."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "recode_plan_dump.c")
CARRY, DEC = 0, 1


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", str(exe)], check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("rplan"), "dump", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("rplan_san"), "dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, streams, block, segs, block_cap=None, tails_max=0, slices=()):
    """streams: [(carry_off, carry_len, failed)]; segs: [(stream, start, samples, ok)].  block_cap defaults to exactly
    the blocks the call makes.  Returns a dict of the printed tables."""
    if block_cap is None:
        block_cap = model(streams, block, segs)["nblocks"]
    words = [len(streams), block, len(segs), block_cap, tails_max, len(slices)]
    for row in list(streams) + list(segs) + list(slices):
        words += list(row)
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    out = dict(P=[], C=[], S=[], B=[], L=[], T=[], refused=False)
    for line in p.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        v = tuple(map(int, w[1:]))
        if w[0] == "E":
            out["refused"] = True
        elif w[0] == "N":
            out["nblocks"], out["nbp"], out["ncp"], out["carry_total"] = v
        elif w[0] == "B":
            out["B"] = list(v)
        elif w[0] in "PCS":
            out[w[0]].append(v)
        elif w[0] == "L":
            out["L"].append([])
        elif w[0] == "Q":
            out["L"][-1].append(v)
        elif w[0] == "T":
            out["T"].append(dict(n=v[0], np=v[1], next=v[2], Z=[], Y=[]))
        elif w[0] in "ZY":
            out["T"][-1][w[0]].append(v)
    return out


def expand(pieces):
    """A piece table as the list of (buf, source sample) it puts at destination 0, 1, 2, ...; checks that it is sorted,
    has counts of at least 1 and tiles its destination exactly."""
    at, out = 0, []
    for buf, count, src, dst in pieces:
        assert count >= 1 and dst == at and buf in (CARRY, DEC), pieces
        out += [(buf, src + i) for i in range(count)]
        at += count
    return out


def model(streams, block, segs):
    """The same step, sample by sample."""
    blocks, block_stream, carry, after = [], [], [], []
    for s, (off, ln, failed) in enumerate(streams):
        mine = [] if failed else [(CARRY, off + i) for i in range(ln)]
        bad = bool(failed)
        for t, start, n, ok in segs:
            if t != s or bad:
                continue
            if not ok:
                bad = True
                continue
            mine += [(DEC, start + i) for i in range(max(n, 0))]
        nb = len(mine) // block
        blocks += mine[:nb * block]
        block_stream += [s] * nb
        rest = [] if bad else mine[nb * block:]
        after.append((len(carry), len(rest), int(bad)))
        carry += rest
    return dict(nblocks=len(block_stream), blocks=blocks, B=block_stream, carry=carry, S=after)


def check(got, streams, block, segs):
    want = model(streams, block, segs)
    assert not got["refused"]
    assert expand(got["P"]) == want["blocks"] and got["B"] == want["B"] and got["nblocks"] == want["nblocks"]
    assert expand(got["C"]) == want["carry"] and got["S"] == want["S"] and got["carry_total"] == len(want["carry"])
    assert len(got["P"]) == got["nbp"] <= len(streams) + len(segs) and len(got["C"]) == got["ncp"] <= len(streams) + len(segs)
    assert all(ln < block for _, ln, _ in got["S"])


def test_a_stream_with_carry_and_no_new_samples(plain):
    """It is copied to the new carry buffer as it is, behind stream 0's; neither makes a block."""
    streams, segs = [(0, 5, 0), (5, 7, 0)], [(0, 100, 2, 1)]
    got = run(plain, streams, 16, segs)
    assert got["nblocks"] == 0 and got["P"] == [] and got["B"] == []
    assert got["C"] == [(CARRY, 5, 0, 0), (DEC, 2, 100, 5), (CARRY, 7, 5, 7)]
    assert got["S"] == [(0, 7, 0), (7, 7, 0)] and got["carry_total"] == 14
    check(got, streams, 16, segs)


def test_carry_plus_two_segments_make_one_block_with_a_remainder(plain):
    streams, segs = [(0, 5, 0)], [(0, 40, 6, 1), (0, 200, 9, 1)]
    got = run(plain, streams, 16, segs)
    # 5 + 6 + 9 = 20: the block takes the carry, the first segment and 5 of the second; 4 stay
    assert got["P"] == [(CARRY, 5, 0, 0), (DEC, 6, 40, 5), (DEC, 5, 200, 11)] and got["B"] == [0]
    assert got["C"] == [(DEC, 4, 205, 0)] and got["S"] == [(0, 4, 0)]
    check(got, streams, 16, segs)


def test_exactly_one_block_and_no_remainder(plain):
    streams, segs = [(0, 6, 0)], [(0, 64, 10, 1)]
    got = run(plain, streams, 16, segs)
    assert got["P"] == [(CARRY, 6, 0, 0), (DEC, 10, 64, 6)] and got["B"] == [0]
    assert got["C"] == [] and got["S"] == [(0, 0, 0)] and got["carry_total"] == 0
    check(got, streams, 16, segs)


def test_several_streams_interleaved(plain):
    """Round-robin segments: blocks come stream by stream, each stream's samples in order; two segments that lie back
    to back in the decoded buffer are one piece."""
    streams = [(0, 2, 0), (2, 0, 0), (2, 3, 0)]
    segs = [(0, 0, 8, 1), (1, 8, 8, 1), (2, 16, 8, 1), (0, 24, 8, 1), (1, 32, 8, 1), (2, 40, 8, 1), (2, 48, 1, 1)]
    got = run(plain, streams, 8, segs)
    assert got["B"] == [0, 0, 1, 1, 2, 2]
    assert got["P"] == [(CARRY, 2, 0, 0), (DEC, 8, 0, 2), (DEC, 6, 24, 10), (DEC, 8, 8, 16), (DEC, 8, 32, 24),
                        (CARRY, 3, 2, 32), (DEC, 8, 16, 35), (DEC, 5, 40, 43)]
    assert got["C"] == [(DEC, 2, 30, 0), (DEC, 4, 45, 2)]      # stream 2: 3 of 40.. and the one at 48, back to back
    assert got["S"] == [(0, 2, 0), (2, 0, 0), (2, 4, 0)]
    check(got, streams, 8, segs)


def test_a_failed_segment_in_the_middle_of_a_batch(plain):
    """Stream 1's second segment is bad: its carry and first segment still make a whole block, nothing behind the bad
    segment is taken, its carry is dropped and it is named failed; streams 0 and 2 are as if it were not there."""
    streams = [(0, 1, 0), (1, 3, 0), (4, 2, 0)]
    segs = [(1, 0, 6, 1), (0, 6, 7, 1), (1, 13, 8, 0), (2, 21, 5, 1), (1, 26, 8, 1)]
    got = run(plain, streams, 8, segs)
    assert got["B"] == [0, 1]
    assert got["P"] == [(CARRY, 1, 0, 0), (DEC, 7, 6, 1), (CARRY, 3, 1, 8), (DEC, 5, 0, 11)]
    assert got["C"] == [(CARRY, 2, 4, 0), (DEC, 5, 21, 2)]
    assert got["S"] == [(0, 0, 0), (0, 0, 1), (0, 7, 0)]
    check(got, streams, 8, segs)
    # a stream that comes in failed gives nothing and keeps nothing, whatever its segments say
    again = run(plain, [(0, 0, 0), (0, 0, 1), (0, 7, 0)], 8, [(1, 0, 8, 1), (2, 8, 1, 1)])
    assert again["B"] == [2] and again["P"] == [(CARRY, 7, 0, 0), (DEC, 1, 8, 7)] and again["S"] == [(0, 0, 0), (0, 0, 1), (0, 0, 0)]


def test_a_block_size_of_one(plain):
    """Every sample is a block; no carry ever."""
    streams, segs = [(0, 0, 0), (0, 0, 0)], [(1, 0, 3, 1), (0, 3, 2, 1)]
    got = run(plain, streams, 1, segs)
    assert got["B"] == [0, 0, 1, 1, 1] and got["P"] == [(DEC, 2, 3, 0), (DEC, 3, 0, 2)] and got["C"] == []
    check(got, streams, 1, segs)


def test_too_many_blocks_change_nothing(plain):
    streams, segs = [(0, 5, 0), (5, 1, 0)], [(0, 0, 30, 1), (1, 30, 2, 0)]
    got = run(plain, streams, 8, segs, block_cap=3)           # 35 samples are 4 blocks
    assert got["refused"] and got["S"] == streams
    assert run(plain, streams, 8, segs, block_cap=4)["B"] == [0] * 4


def test_slices_of_the_block_table(plain):
    """A chunk of an encode call gathers part of the destination: the pieces cut at the chunk's ends and re-based."""
    streams, segs = [(0, 5, 0)], [(0, 40, 6, 1), (0, 200, 21, 1)]      # 32 samples: 5 | 6 | 21
    got = run(plain, streams, 16, segs, slices=[(0, 16), (16, 32)])
    assert got["L"] == [[(CARRY, 5, 0, 0), (DEC, 6, 40, 5), (DEC, 5, 200, 11)], [(DEC, 16, 205, 0)]]
    got = run(plain, streams, 16, segs, slices=[(3, 7), (7, 8), (30, 32)])
    assert got["L"] == [[(CARRY, 2, 3, 0), (DEC, 2, 40, 2)], [(DEC, 1, 42, 0)], [(DEC, 2, 219, 0)]]


def test_tails(plain):
    """At the end every good stream's carry is one block of a ragged batch, at most tails_max a batch; carries that lie
    back to back in the carry buffer are one piece."""
    streams = [(0, 3, 0), (3, 0, 0), (3, 4, 1), (3, 5, 0), (8, 1, 0)]
    got = run(plain, streams, 16, [], tails_max=2)
    assert [(t["n"], t["Z"], t["Y"]) for t in got["T"]] == [
        (2, [(3, 0), (5, 3)], [(CARRY, 8, 0, 0)]), (1, [(1, 4)], [(CARRY, 1, 8, 0)])]
    assert got["T"][-1]["next"] == 5


def random_calls():
    r = np.random.RandomState(20261019)
    out = []
    for _ in range(80):
        ns = int(r.randint(1, 7))
        block = int(r.choice([1, 2, 7, 16, 96]))
        streams, off = [], 0
        for _ in range(ns):
            failed = int(r.rand() < 0.15)
            ln = 0 if failed else int(r.randint(0, block))
            streams.append((off, ln, failed))
            off += ln
        segs, at = [], 0
        for _ in range(int(r.randint(0, 14))):
            n = int(r.choice([0, 1, 2, 5, 16, 64, 200]))
            segs.append((int(r.randint(0, ns)), at, n, int(r.rand() > 0.12)))
            at += n
        out.append((streams, block, segs))
    return out


def walk(exe, streams, block, segs):
    want = model(streams, block, segs)
    total = want["nblocks"] * block
    cuts = sorted({0, total, total // 3, (total // 3) * 2})
    slices = list(zip(cuts[:-1], cuts[1:]))
    got = run(exe, streams, block, segs, tails_max=3, slices=slices)
    check(got, streams, block, segs)
    # the slices put together are the table, each re-based to 0
    parts = [expand(q) for q in got["L"]]
    assert [x for part in parts for x in part] == want["blocks"]
    assert [len(part) for part in parts] == [hi - lo for lo, hi in slices]
    # every good stream's carry appears once in the tails, in stream order
    tails = [z for t in got["T"] for z in t["Z"]]
    assert tails == [(ln, s) for s, (_, ln, failed) in enumerate(got["S"]) if ln and not failed]
    assert [x for t in got["T"] for x in expand(t["Y"])] == [(CARRY, i) for i in range(got["carry_total"])]
    return got


def test_random_calls_agree_with_the_model(plain):
    for streams, block, segs in random_calls():
        walk(plain, streams, block, segs)


def test_streams_stay_whole_across_many_steps(plain):
    """Several steps in a row, each fed the carries of the one before: every stream's samples come out once and in
    order across the blocks of all steps and the last carry."""
    r = np.random.RandomState(7)
    ns, block = 4, 16
    streams = [(0, 0, 0)] * ns
    carry_ids = []                                     # what the carry buffer holds: (stream, running sample index)
    fed = [0] * ns
    seen = [[] for _ in range(ns)]
    for _ in range(12):
        segs, dec_ids, at = [], [], 0
        for _ in range(int(r.randint(1, 6))):
            s, n = int(r.randint(0, ns)), int(r.choice([1, 3, 16, 40]))
            segs.append((s, at, n, 1))
            dec_ids += [(s, fed[s] + i) for i in range(n)]
            fed[s] += n
            at += n
        got = run(plain, streams, block, segs)
        look = lambda x: carry_ids[x[1]] if x[0] == CARRY else dec_ids[x[1]]
        blocks = [look(x) for x in expand(got["P"])]
        for b, s in enumerate(got["B"]):
            part = blocks[b * block:(b + 1) * block]
            assert all(t == s for t, _ in part)
            seen[s] += [i for _, i in part]
        carry_ids = [look(x) for x in expand(got["C"])]
        streams = got["S"]
    for s in range(ns):
        off, ln, _ = streams[s]
        assert seen[s] + [i for _, i in carry_ids[off:off + ln]] == list(range(fed[s]))


def test_every_case_again_under_the_sanitizers(plain, sanitized):
    """The same program with -fsanitize=address,undefined: it ends cleanly (a report aborts it) with the same output."""
    named = [
        ([(0, 5, 0), (5, 7, 0)], 16, [(0, 100, 2, 1)]),
        ([(0, 5, 0)], 16, [(0, 40, 6, 1), (0, 200, 9, 1)]),
        ([(0, 6, 0)], 16, [(0, 64, 10, 1)]),
        ([(0, 2, 0), (2, 0, 0), (2, 3, 0)], 8, [(0, 0, 8, 1), (1, 8, 8, 1), (2, 16, 8, 1), (0, 24, 8, 1), (1, 32, 8, 1),
                                                  (2, 40, 8, 1), (2, 48, 1, 1)]),
        ([(0, 1, 0), (1, 3, 0), (4, 2, 0)], 8, [(1, 0, 6, 1), (0, 6, 7, 1), (1, 13, 8, 0), (2, 21, 5, 1), (1, 26, 8, 1)]),
        ([(0, 0, 0), (0, 0, 0)], 1, [(1, 0, 3, 1), (0, 3, 2, 1)]),
        ([(0, 0, 0)], 16, []),
    ]
    for streams, block, segs in named + random_calls():
        assert walk(sanitized, streams, block, segs) == walk(plain, streams, block, segs)
    refused = run(sanitized, [(0, 5, 0), (5, 1, 0)], 8, [(0, 0, 30, 1), (1, 30, 2, 0)], block_cap=3)
    assert refused["refused"] and refused["S"] == [(0, 5, 0), (5, 1, 0)]
