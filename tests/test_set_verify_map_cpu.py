"""The map a stream set uses when a chunk fails verification (flake_amd/host/host_internal.h, fa_block_of_frame): the
verifier's first failing frame index -> the block of the chunk that frame lies in, by the prefix sum of block_frames;
the block names the stream.  The encoder cannot be made to fail from outside, so the C function is run here on its
own: a host program includes the header and prints its answers.  Runs without a GPU.

block_of_frame() below is the numpy expression test_gpu_set_vbs.py holds a real verdict to; the two are held to each
other on random tables."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "flake_amd", "host")


def block_of_frame(block_frames, frame):
    """The block (of len(block_frames) blocks, every entry >= 1) that holds frame `frame` of the chunk, or -1."""
    ends = np.cumsum(block_frames)
    if frame < 0 or len(ends) == 0 or frame >= ends[-1]:
        return -1
    return int(np.searchsorted(ends, frame, side="right"))


def random_tables():
    r = np.random.RandomState(20241018)
    return [r.randint(1, 9, r.randint(1, 65)).astype(np.int32) for _ in range(40)]


# name: (block_frames or None, cnt, [(frame, expected block)])
CASES = {
    "blocks of 1 3 2 1": ([1, 3, 2, 1], 4, [(0, 0), (1, 1), (3, 1), (4, 2), (5, 2), (6, 3), (7, -1), (-1, -1)]),
    "a zero entry ends the search": ([2, 0, 3], 3, [(0, 0), (1, 0), (2, -1), (3, -1), (4, -1)]),
    "a negative entry ends the search": ([1, -2, 3], 3, [(0, 0), (1, -1), (2, -1)]),
    "null table, four blocks": (None, 4, [(0, 0), (1, 1), (2, 2), (3, 3), (4, -1), (-1, -1)]),
    "no blocks": (None, 0, [(0, -1)]),
}
# a chunk that starts at block b0 = 3 of the call's table {5, 5, 5, 2, 1, 4}: the map sees the chunk's part only
B0_TABLE, B0, B0_CNT = [5, 5, 5, 2, 1, 4], 3, 3
B0_EXPECT = [(0, 0), (1, 0), (2, 1), (3, 2), (6, 2), (7, -1)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """Every query of the module in one run of one program: {case name: [answers]}."""
    tmp = tmp_path_factory.mktemp("verify_map")
    body, queries = [], {}

    def add(name, table, first, cnt, frames):
        k = len(queries)
        queries[name] = len(frames)
        if table is not None:
            body.append(f"    static const int32_t t{k}[] = {{{', '.join(map(str, table))}}};\n")
        ptr = f"t{k} + {first}" if table is not None else "NULL"
        body.append(f"    static const long long q{k}[] = {{{', '.join(map(str, frames))}}};\n"
                    f"    for (int i = 0; i < {len(frames)}; i++) printf(\"%d\\n\", fa_block_of_frame(q{k}[i], {ptr}, {cnt}));\n")

    for name, (table, cnt, pairs) in CASES.items():
        add(name, table, 0, cnt, [f for f, _ in pairs])
    add("b0", B0_TABLE, B0, B0_CNT, [f for f, _ in B0_EXPECT])
    for i, t in enumerate(random_tables()):
        add(f"random {i}", list(t), 0, len(t), list(range(-1, int(t.sum()) + 2)))
    src = tmp / "map.c"
    src.write_text('#include <stdio.h>\n#include "host_internal.h"\nint main(void)\n{\n' + "".join(body) +
                   "    return 0;\n}\n")
    exe = tmp / "map"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", HOST, str(src), "-o", str(exe)], check=True,
                   capture_output=True, timeout=120)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    got, pos = {}, 0
    for name, n in queries.items():
        got[name] = out[pos:pos + n]
        pos += n
    assert pos == len(out)
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_map_answers(answers, name):
    assert answers[name] == [blk for _, blk in CASES[name][2]], name


def test_chunk_that_starts_inside_the_call(answers):
    assert answers["b0"] == [blk for _, blk in B0_EXPECT]


def test_numpy_expression_agrees_on_random_tables(answers):
    for i, t in enumerate(random_tables()):
        frames = range(-1, int(t.sum()) + 2)
        assert answers[f"random {i}"] == [block_of_frame(t, f) for f in frames], (i, list(t))
