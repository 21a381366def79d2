"""The planner of flake_amd_set_encode_rows (flake_amd/host/rows_plan.h) on its own: how the rows of a planar batch become
the whole blocks and the short blocks of a stream set's two calls, as K12's piece tables, and how a chunk's part of a
table is sliced out.  It makes no HIP call, so a host program (tools/rows_plan_dump.c) runs it here without a GPU and
prints its tables -- once built plain, once with -fsanitize=address,undefined, every array exactly as large as promised.
The expected tables are written out by hand for the named cases; random calls are held against a model in Python that
moves sample by sample."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "rows_plan_dump.c")
B = 256


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, "-I", os.path.join(ROOT, "include"),
                    SRC, "-o", str(exe)], check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("rowsplan"), "dump", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return build(tmp_path_factory.mktemp("rowsplan_san"), "dump_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run(exe, rows, block, wslices=(), sslices=()):
    """rows: [(len, stream)]; slices: [(lo, hi)].  Returns a dict of the printed tables."""
    words = [len(rows), block, len(wslices), len(sslices)]
    for row in list(rows) + list(wslices) + list(sslices):
        words += list(row)
    p = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    out = dict(W=[], P=[], F=[], Z=[], S=[], L=[], M=[], refused=False)
    for line in p.stdout.split("\n"):
        w = line.split()
        if not w:
            continue
        v = tuple(map(int, w[1:]))
        if w[0] == "E":
            out["refused"] = True
        elif w[0] == "N":
            out["nwhole"], out["nwp"], out["nshort"] = v
        elif w[0] in "WF":
            out[w[0]] = list(v)
        elif w[0] in "PZS":
            out[w[0]].append(v)
        elif w[0] in "LM":
            out[w[0]].append([])
        elif w[0] == "Q":
            out["L"][-1].append(v)
        elif w[0] == "R":
            out["M"][-1].append(v)
    return out


def expand(pieces):
    """A piece table (row, count, col, dst) as the list of (row, column) it puts at destination 0, 1, 2, ...; checks that
    it is sorted, has counts of at least 1 and tiles its destination exactly."""
    at, out = 0, []
    for row, count, col, dst in pieces:
        assert count >= 1 and dst == at and col >= 0, pieces
        out += [(row, col + i) for i in range(count)]
        at += count
    return out


def model(rows, block):
    """Sample by sample: where every sample of every whole block and of every short block comes from."""
    whole, wstream, short, z, first = [], [], [], [], []
    for r, (n, s) in enumerate(rows):
        first.append(len(wstream))
        for b in range(n // block):
            wstream.append(s)
            whole += [(r, b * block + i) for i in range(block)]
        if n % block:
            z.append((n % block, s, r))
            short += [(r, (n // block) * block + i) for i in range(n % block)]
    first.append(len(wstream))
    return dict(whole=whole, W=wstream, short=short, Z=z, F=first)


def check_against_model(got, rows, block, wslices=(), sslices=()):
    m = model(rows, block)
    assert not got["refused"]
    assert got["nwhole"] == len(m["W"]) and got["W"] == m["W"] and got["F"] == m["F"]
    assert got["nshort"] == len(m["Z"]) and got["Z"] == m["Z"]
    assert got["nwp"] == len(got["P"]) == sum(1 for n, _ in rows if n >= block)      # one piece per run of blocks
    assert len(got["S"]) == got["nshort"]
    assert expand(got["P"]) == m["whole"] and expand(got["S"]) == m["short"]
    for slices, parts, full in ((wslices, got["L"], m["whole"]), (sslices, got["M"], m["short"])):
        assert len(parts) == len(slices)
        for (lo, hi), part in zip(slices, parts):
            assert expand(part) == full[max(lo, 0):max(min(hi, len(full)), 0)], (lo, hi)


NAMED = [(0, 4), (1, 0), (B - 1, 1), (B, 2), (B + 1, 3), (3 * B, 5), (3 * B + 17, 6)]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_named_lengths_written_out(which, request):
    exe = request.getfixturevalue(which)
    got = run(exe, NAMED, B, wslices=[(0, 8 * B)], sslices=[(0, 1 + 255 + 1 + 17)])
    assert (got["nwhole"], got["nwp"], got["nshort"]) == (8, 4, 4)
    assert got["W"] == [2, 3, 5, 5, 5, 6, 6, 6]
    assert got["F"] == [0, 0, 0, 0, 1, 2, 5, 8]
    # (row, count, col, dst): one piece per row that has whole blocks, spanning all of them
    assert got["P"] == [(3, B, 0, 0), (4, B, 0, B), (5, 3 * B, 0, 2 * B), (6, 3 * B, 0, 5 * B)]
    # (size, stream, row)
    assert got["Z"] == [(1, 0, 1), (B - 1, 1, 2), (1, 3, 4), (17, 6, 6)]
    assert got["S"] == [(1, 1, 0, 0), (2, B - 1, 0, 1), (4, 1, B, B), (6, 17, 3 * B, B + 1)]
    assert got["L"] == [got["P"]] and got["M"] == [got["S"]]
    check_against_model(got, NAMED, B, [(0, 8 * B)], [(0, 274)])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_nothing_at_all(which, request):
    exe = request.getfixturevalue(which)
    for rows in ([], [(0, 0)], [(0, 3), (0, 3)]):
        got = run(exe, rows, B, wslices=[(0, 0), (0, 100)], sslices=[(0, 100)])
        assert (got["nwhole"], got["nwp"], got["nshort"]) == (0, 0, 0)
        assert got["W"] == [] and got["P"] == [] and got["S"] == [] and got["L"] == [[], []] and got["M"] == [[]]
        assert got["F"] == [0] * (len(rows) + 1)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_two_rows_of_one_stream(which, request):
    """Rows 0 and 2 are of stream 7: its whole blocks come in row order, row 2's short block behind all whole blocks."""
    exe = request.getfixturevalue(which)
    rows = [(2 * B, 7), (B, 1), (B + 44, 7)]
    got = run(exe, rows, B)
    assert got["W"] == [7, 7, 1, 7] and got["F"] == [0, 2, 3, 4]
    assert got["P"] == [(0, 2 * B, 0, 0), (1, B, 0, 2 * B), (2, B, 0, 3 * B)]
    assert got["Z"] == [(44, 7, 2)] and got["S"] == [(2, 44, B, 0)]
    check_against_model(got, rows, B)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_slices_cut_a_piece_at_a_chunk_border(which, request):
    """Chunks of three blocks over rows of 2, 5 and 1 blocks: the second row's piece is cut twice, and every slice is
    re-based to 0."""
    exe = request.getfixturevalue(which)
    rows = [(2 * B + 5, 0), (5 * B + 100, 1), (B + 7, 2)]
    wsl = [(0, 3 * B), (3 * B, 6 * B), (6 * B, 8 * B)]
    ssl = [(0, 105), (105, 112)]                                           # two short blocks, then the third
    got = run(exe, rows, B, wslices=wsl, sslices=ssl)
    assert got["L"] == [[(0, 2 * B, 0, 0), (1, B, 0, 2 * B)],
                        [(1, 3 * B, B, 0)],
                        [(1, B, 4 * B, 0), (2, B, 0, B)]]
    assert got["M"] == [[(0, 5, 2 * B, 0), (1, 100, 5 * B, 5)], [(2, 7, B, 0)]]
    check_against_model(got, rows, B, wsl, ssl)
    # borders inside a block, an empty slice and one that reaches past the end
    wsl = [(0, 10), (10, 10), (10, 2 * B + 1), (2 * B + 1, 7 * B + 255), (7 * B + 255, 9 * B)]
    ssl = [(0, 4), (4, 6), (6, 111), (111, 500)]
    check_against_model(run(exe, rows, B, wslices=wsl, sslices=ssl), rows, B, wsl, ssl)


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_refusals(which, request):
    exe = request.getfixturevalue(which)
    assert run(exe, [(5, 0)], 0)["refused"]                              # no block size
    assert run(exe, [(-1, 0)], B)["refused"]                             # a negative length
    assert run(exe, [(2 ** 31, 0)], B)["refused"]                        # a length no piece's count holds
    assert run(exe, [(2 ** 31 - 1, 0)] * 3, 1)["refused"]                # more blocks than an int holds
    assert not run(exe, [(2 ** 31 - 1, 0)], 2 ** 30)["refused"]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_random_calls_against_the_model(which, request):
    exe = request.getfixturevalue(which)
    r = np.random.RandomState(5 if which == "plain" else 6)
    for _ in range(40):
        block = int(r.choice([1, 2, 16, 64, 100]))
        nrows = int(r.randint(0, 9))
        rows = [(int(r.choice([0, 1, block - 1, block, block + 1, 3 * block, r.randint(0, 6 * block)])), int(r.randint(0, 4)))
                for _ in range(nrows)]
        m = model(rows, block)

        def cuts(total):
            at, out = 0, []
            while at < total:
                step = int(r.randint(1, 3 * block + 2))
                out.append((at, min(at + step, total)))
                at += step
            return out

        wsl, ssl = cuts(len(m["whole"])), cuts(len(m["short"]))
        check_against_model(run(exe, rows, block, wslices=wsl, sslices=ssl), rows, block, wsl, ssl)
