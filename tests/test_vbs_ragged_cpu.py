"""The block lookup of the verifier's ragged block-table mode (flake_amd/csrc/vbs_block_lookup.h): which block of a
batch of blocks of different lengths a sample position lies in.  K5 and api.hip share the header; here a host program
includes it (gcc, no HIP) and its answers are held to numpy.searchsorted on seeded random length tables -- lengths of 1,
one block only, and positions at every block boundary and at the total among them.  The new entries are also checked
to be exported and to refuse null arguments.  Runs without a GPU."""
import os
import subprocess

import numpy as np
import pytest

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flake_amd", "csrc")


def tables():
    r = np.random.RandomState(20261018)
    out = [np.array([1]), np.array([1152]), np.array([1, 1, 1, 1]), np.array([65535, 1, 65535])]
    for _ in range(40):
        n = int(r.randint(1, 200))
        t = r.randint(1, 4097, n)
        t[r.randint(0, n, max(n // 8, 1))] = 1                   # lengths of 1 among them
        out.append(t)
    return out


def positions(table, r):
    start = np.concatenate([[0], np.cumsum(table)])
    edge = np.concatenate([start, start - 1, start + 1])
    rand = r.randint(-2, int(start[-1]) + 3, 64)
    return start, np.concatenate([edge, rand, [-1, -5, int(start[-1]) + 1000]])


def expected(start, s):
    """The block b with start[b] <= s < start[b + 1]; nblocks at or behind the end, -1 before the batch."""
    if s < 0:
        return -1
    return int(np.searchsorted(start[1:], s, side="right"))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("block_lookup")
    r = np.random.RandomState(7)
    body, cases = [], []
    for k, t in enumerate(tables()):
        start, pos = positions(t, r)
        cases.append((start, pos))
        body.append(f"    static const long long s{k}[] = {{{', '.join(map(str, start))}}};\n"
                    f"    static const long long q{k}[] = {{{', '.join(map(str, pos))}}};\n"
                    f"    for (int i = 0; i < {len(pos)}; i++) printf(\"%d\\n\", fhip_block_lookup(s{k}, {len(t)}, q{k}[i]));\n")
    src = tmp / "lookup.c"
    src.write_text('#include <stdio.h>\n#include "vbs_block_lookup.h"\nint main(void)\n{\n' + "".join(body) +
                   "    return 0;\n}\n")
    exe = tmp / "lookup"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True,
                   capture_output=True, timeout=120)
    out = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    got, at = [], 0
    for start, pos in cases:
        got.append(out[at:at + len(pos)])
        at += len(pos)
    assert at == len(out)
    return cases, got


def test_lookup_equals_searchsorted(answers):
    cases, got = answers
    for (start, pos), g in zip(cases, got):
        assert g == [expected(start, int(s)) for s in pos], list(np.diff(start))


def test_every_boundary_and_the_total(answers):
    cases, got = answers
    for (start, pos), g in zip(cases, got):
        nb = len(start) - 1
        by_pos = dict(zip(map(int, pos), g))
        for b in range(nb):
            assert by_pos[int(start[b])] == b                    # a block's first sample is its own
            assert by_pos[int(start[b + 1]) - 1] == b            # ... and so is its last
        assert by_pos[int(start[nb])] == nb                      # the total lies in no block


NEW = ("fhip_encode_blocks_vbs_ragged_numbered", "fhip_vbs_split_ragged", "fhip_verify_frames_blocks_ragged",
       "fhip_verify_frames_blocks_ragged_dev")


def test_new_entries_are_exported_and_declared():
    lib = flake_amd.load_library()
    header = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in flake_amd.ABI_SYMBOLS and f"FHIP_API int {name}(" in header, name
    assert lib.fhip_encode_blocks_vbs_ragged_numbered(None, None, 0, None, None, None, 0, None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_vbs_split_ragged(None, None, 0, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_blocks_ragged(None, None, None, 0, None, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_blocks_ragged_dev(None, None, None, 0, None, None) == flake_amd.E_INVALID
    host = flake_amd.load_host_library()
    assert host.flake_amd_set_device_batches(None) == -1
    for name in ("encode_blocks_vbs_ragged_numbered", "verify_frames_blocks_ragged", "vbs_split_ragged"):
        assert callable(getattr(flake_amd.Encoder, name))
    assert callable(flake_amd.StreamSet.device_batches)
