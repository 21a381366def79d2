"""The row bookkeeping of span rows (flake_amd/host/span_rows_plan.h) against a Python model that walks the rows one by
one: how many rows a span has, where every span's rows lie, what each row holds at the end and what K13 is told of a
batch's segments.  tools/span_rows_plan_dump.c runs the header on cases from standard input; built plain and with
-fsanitize=address,undefined, every table at exactly the size the header asks for.  Swept: count 0 .. 40, row_len 1 .. 9,
hop 1 .. 12, and count 2^40.  Every row holds at least one asked sample, and for hop <= row_len the rows cover
[0, count).  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "span_rows_plan_dump.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COUNTS, ROW_LENS, HOPS = range(0, 41), range(1, 10), range(1, 13)
BIG = 2 ** 40


def build(tmp, name, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, SRC, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("srplan")
    return {"plain": build(tmp, "dump", []), "san": build(tmp, "dump_san", SAN)}


# ---- the model: the rows one by one ------------------------------------------------------------------------------------
def row_starts(count, row_len, hop):
    """Where a span's rows begin: the rows j with j * hop < count whose predecessor has not already reached the end."""
    starts = []
    while len(starts) * hop < count and (not starts or starts[-1] + row_len < count):
        starts.append(len(starts) * hop)
    return starts


def held(delivered, start, row_len):
    return -1 if delivered < 0 else min(max(delivered - start, 0), row_len)


def delivered_of(s, count):
    """What span s is said to have delivered: all, half, nothing, or it failed."""
    return (count, count // 2, 0, -1)[s % 4]


def run(exe, cases):
    text = "\n".join(" ".join(map(str, [row_len, hop, cap, len(spans), *[x for sp in spans for x in sp], len(segs), *segs]))
                     for row_len, hop, cap, spans, segs in cases)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    out, cur = [], None
    for line in p.stdout.split("\n"):
        if line.startswith("C"):
            cur = {}
            out.append(cur)
        if line.strip():
            cur[line[0]] = line.split()[1:]
    assert len(out) == len(cases)
    return out


@pytest.mark.parametrize("leg", ["plain", "san"])
def test_the_sweep_against_the_model(exes, leg):
    cases = []
    for row_len in ROW_LENS:
        for hop in HOPS:
            spans = [(c, delivered_of(s, c)) for s, c in enumerate(COUNTS)]
            segs = [s % len(spans) for s in range(0, 3 * len(spans), 7)] + [-1, 0, -1]
            cases.append((row_len, hop, 10 ** 6, spans, segs))
    for (row_len, hop, _, spans, segs), got in zip(cases, run(exes[leg], cases)):
        starts = [row_starts(c, row_len, hop) for c, _ in spans]
        for (c, _), st in zip(spans, starts):
            # what the rows are for: every row holds an asked sample, and without gaps between rows nothing is left out
            assert all(s < c for s in st), (c, row_len, hop)
            if hop <= row_len:
                covered = set()
                for s in st:
                    covered |= set(range(s, min(s + row_len, c)))
                assert covered == set(range(c)), (c, row_len, hop)
        assert [int(x) for x in got["C"]] == [len(st) for st in starts], (row_len, hop)
        first = [0]
        for st in starts:
            first.append(first[-1] + len(st))
        assert [int(x) for x in got["F"]] == [first[-1], *first], (row_len, hop)
        want = [held(d, s, row_len) for (_, d), st in zip(spans, starts) for s in st]
        assert [int(x) for x in got["L"]] == want, (row_len, hop)
        assert got["B"] == [("-1:0" if s < 0 else f"{first[s]}:{len(starts[s])}") for s in segs], (row_len, hop)


@pytest.mark.parametrize("leg", ["plain", "san"])
def test_big_counts_bad_arguments_and_the_room(exes, leg):
    def closed(c, row_len, hop):
        return min(-(-c // hop), 1 + -(-max(c - row_len, 0) // hop)) if c else 0
    cases = [(row_len, hop, 2 ** 40, [(BIG, BIG)], []) for row_len in (1, 9, 4096, BIG, BIG + 5) for hop in (1, 12, 2 ** 31 - 1)]
    for (row_len, hop, _, _, _), got in zip(cases, run(exes[leg], cases)):
        assert int(got["C"][0]) == closed(BIG, row_len, hop), (row_len, hop)
        # a call has no more than 2^31 - 1 rows, whatever room the caller has
        assert int(got["F"][0]) == (closed(BIG, row_len, hop) if closed(BIG, row_len, hop) < 2 ** 31 else -1), (row_len, hop)
    # the closed form is the model's wherever the model can walk
    assert all(closed(c, r, h) == len(row_starts(c, r, h)) for c in COUNTS for r in ROW_LENS for h in HOPS)
    bad = run(exes[leg], [(4, 0, 100, [(8, 8)], []), (0, 2, 100, [(8, 8)], []), (4, 2 ** 31, 100, [(8, 8)], []),
                          (4, 2, 100, [(8, 8), (-1, 0)], []), (4, 2, -1, [], [])])
    assert [g["F"] for g in bad] == [["-1"]] * 5
    assert [g["C"] for g in bad[:4]] == [["-1"], ["-1"], ["-1"], ["3", "-1"]]
    # rows_cap: exactly enough is enough, one short is refused; no span at all is no row
    spans = [(8, 8), (0, 0), (3, 3), (9, 9)]                  # 3 + 0 + 1 + 4 rows of (4, 2)
    room = run(exes[leg], [(4, 2, 8, spans, [3, 1]), (4, 2, 7, spans, []), (4, 2, 0, [], []), (4, 2, 0, [(0, 0)], [0])])
    assert room[0]["F"] == ["8", "0", "3", "3", "4", "8"] and room[0]["B"] == ["4:4", "3:0"]
    assert room[0]["L"] == ["4", "4", "4", "3", "4", "4", "4", "3"]
    assert room[1]["F"] == ["-1"] and room[2]["F"] == ["0", "0"] and room[3]["F"] == ["0", "0", "0"]
