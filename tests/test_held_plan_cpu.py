"""The window planner over a held store's table of heads (flake_amd/host/held_plan.h) against the same planner over the
runs' bytes (decode_window_plan.h): one selection, one batch rule, two header accessors that must probe the same frames
in the same order.  tools/held_plan_dump.c runs both on a call and prints both; here the two halves are held to each
other field for field on seeded random runs -- fixed and variable blocks, broken headers at frames the bisection probes
and at frames it does not, windows before, inside, across the end of and behind the run and of count 0, max_batch 1, 2, 3
and large -- and the bytes half to tools/decode_window_plan_dump.c, whose tables other tests write out by hand.  Built
plain and with -fsanitize=address,undefined (the table leg runs after every run's bytes are freed).  No GPU."""
import os
import random
import subprocess

import pytest

import flacgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")
SRC = os.path.join(ROOT, "tools", "held_plan_dump.c")
OLD = os.path.join(ROOT, "tools", "decode_window_plan_dump.c")
FMT = (1, 16, 44100, 0)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FAILED = -1


def build(tmp, name, src, extra):
    exe = tmp / name
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", *extra, "-I", HOST, src, "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hplan")
    return {"plain": build(tmp, "dump", SRC, []), "san": build(tmp, "dump_san", SRC, SAN), "old": build(tmp, "old", OLD, [])}


def frame(number, n, vbs=False, broken=False):
    """A frame as far as the planner reads it (test_decode_window_plan_cpu.py's): a mono 16-bit 44.1 kHz header with the
    block size as an 8-bit field, and three bytes that stand for the rest."""
    h = bytes([0xFF, 0xF8 | int(vbs), 0x69, 0x08]) + flacgen.utf8(number) + bytes([n - 1])
    c = flacgen.crc8(h)
    return h + bytes([c ^ (0x55 if broken else 0)]) + b"\0\0\0"


def fixed_run(rng, nframes, block, first_number=0, broken=()):
    last = rng.randrange(1, block + 1)
    return [frame(first_number + k, last if k == nframes - 1 else block, broken=k in broken) for k in range(nframes)]


def variable_run(rng, nframes, start=0, broken=()):
    out, at = [], start
    for k in range(nframes):
        n = rng.randrange(16, 257)
        out.append(frame(at, n, vbs=True, broken=k in broken))
        at += n
    return out, at


def words(windows, max_batch):
    w = [*FMT, max_batch, len(windows)]
    for frames, fixed, first, count in windows:
        w += [len(frames), fixed, first, count, *[len(f) for f in frames], *b"".join(frames)]
    return " ".join(map(str, w))


def run(exe, windows, max_batch):
    p = subprocess.run([exe], input=words(windows, max_batch), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]                # (a sanitizer report ends the program with an error)
    return p.stdout


def legs(text):
    """{"bytes": lines, "table": lines}"""
    out, cur = {}, None
    for line in text.split("\n"):
        if line.startswith("L "):
            cur = out.setdefault(line[2:], [])
        elif line.strip():
            cur.append(tuple(line.split()))
    return out


def probes(nframes, a_target, b_target):
    """The frames the two bisections read for a window whose first frame is a_target and last b_target."""
    seen = [0]
    lo, hi = 0, nframes - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        seen.append(mid)
        if mid <= a_target:
            lo = mid
        else:
            hi = mid - 1
    lo, hi = a_target, nframes - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        seen.append(mid)
        if mid <= b_target:
            lo = mid
        else:
            hi = mid - 1
    return set(seen)


def calls():
    """[(name, windows)]: seeded, so every run of the suite sees the same calls."""
    rng = random.Random(20241)
    out = []
    # windows of every kind on a fixed-block and a variable-block run
    F = fixed_run(rng, 23, 192)
    endF = 22 * 192 + F[-1][-5] + 1
    V, endV = variable_run(rng, 19, start=1000)
    kinds = []
    for run_, fixed, start, end in ((F, 192, 0, endF), (F, 0, 0, endF), (V, 0, 1000, endV), (V, 4096, 1000, endV)):
        mid = (start + end) // 2
        kinds += [(run_, fixed, max(start - 50, 0), 20), (run_, fixed, mid, 1), (run_, fixed, mid, 700),
                  (run_, fixed, start, end - start), (run_, fixed, end - 30, 100), (run_, fixed, end, 5),
                  (run_, fixed, end + 1000, 5), (run_, fixed, mid, 0), (run_[7:], fixed, mid, 300), (run_[-1:], fixed, end - 5, 50),
                  ([], fixed, mid, 5)]
    out.append(("kinds", kinds))
    # random windows on random runs
    rnd = []
    for _ in range(40):
        if rng.random() < 0.5:
            n = rng.randrange(1, 40)
            r = fixed_run(rng, n, 192, first_number=rng.randrange(0, 5))
            fixed, total = rng.choice((0, 192)), (n + 5) * 192
        else:
            r, total = variable_run(rng, rng.randrange(1, 40), start=rng.randrange(0, 3000))
            fixed = 0
        rnd.append((r, fixed, rng.randrange(0, total + 200), rng.randrange(0, 1500)))
    out.append(("random", rnd))
    # a broken header at a frame the bisection probes, and at one it does not
    brk = []
    for nframes, a, b in ((23, 3, 5), (23, 20, 22), (16, 7, 7), (9, 0, 8)):
        seen = probes(nframes, a, b)
        unseen = [k for k in range(nframes) if k not in seen]
        for k in sorted(seen) + unseen[:3]:
            r = fixed_run(rng, nframes, 192, broken=(k,))
            brk.append((r, 192, a * 192 + 7, (b - a) * 192 + 20))
    out.append(("broken", brk))
    return out


CALLS = calls()
BATCHES = (1, 2, 3, 1000)


@pytest.mark.parametrize("max_batch", BATCHES)
@pytest.mark.parametrize("name", [n for n, _ in CALLS])
def test_the_table_plans_what_the_bytes_plan(exes, name, max_batch):
    windows = dict(CALLS)[name]
    text = run(exes["plain"], windows, max_batch)
    both = legs(text)
    assert sorted(both) == ["bytes", "table"]
    assert len([r for r in both["bytes"] if r[0] == "W"]) == len(windows)
    for got, want in zip(both["table"], both["bytes"]):
        assert got == want
    assert len(both["table"]) == len(both["bytes"])
    # the bytes half is the planner every existing caller runs
    old = [tuple(line.split()) for line in run(exes["old"], windows, max_batch).split("\n") if line.strip()]
    assert both["bytes"] == old
    # and the sanitizer build prints the same
    assert run(exes["san"], windows, max_batch) == text


def test_broken_headers_fail_exactly_the_windows_that_probe_them(exes):
    """The cases are not vacuous: with room for the whole sub-run in one batch, a window fails where its probes meet the
    broken frame and nowhere else -- in both halves."""
    windows = dict(CALLS)["broken"]
    both = legs(run(exes["plain"], windows, 1000))
    status = [int(r[1]) for r in both["table"] if r[0] == "W"]
    at = 0
    for nframes, a, b in ((23, 3, 5), (23, 20, 22), (16, 7, 7), (9, 0, 8)):
        seen = probes(nframes, a, b)
        unseen = [k for k in range(nframes) if k not in seen][:3]
        for k in sorted(seen):
            assert status[at] == FAILED, (nframes, a, b, k)
            at += 1
        for k in unseen:
            assert status[at] == 0, (nframes, a, b, k)
            at += 1
    assert at == len(windows) and FAILED in status and 0 in status


def test_a_cut_reads_the_header_behind_it_from_the_table(exes):
    """max_batch 2 cuts a window of eight frames; the broken frame 3 is read by the cut alone, in both halves."""
    rng = random.Random(7)
    r = fixed_run(rng, 10, 192, broken=(3,))
    both = legs(run(exes["plain"], [(r, 192, 200, 1500)], 2))
    assert both["table"] == both["bytes"]
    assert both["table"][0][1] == "0" and both["table"][-1] == ("E", str(FAILED))
