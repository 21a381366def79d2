"""The CPU side of tests/test_gpu_held_stream_order.py: every case's poison conditions hold -- the witness gives three
pairwise different results for versions A, B and C of one geometry, so that work which saw the wrong version cannot
pass -- and the witnesses are what the format and numpy say, not what the entries give."""
import os
import re

import numpy as np
import pytest

import test_gpu_held_stream_order as TH
import test_gpu_stream_order as T
from test_flac_header_cpu import reference


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_device_entry_of_the_held_header_has_a_case():
    """tests/test_stream_order_cases_cpu.py holds include/flakehip.h's device entries to the cases of
    tests/test_gpu_stream_order.py; the held-streams entries are declared in include/flakehip_held.h and have their cases
    in tests/test_gpu_held_stream_order.py: the same condition, on that pair.  The host forms (_held, fhip_hold_frames)
    synchronise before they return and run no work on a stream of their own beside the caller's."""
    text = open(os.path.join(ROOT, "include", "flakehip_held.h")).read()
    names = re.findall(r"FHIP_API\s+[\w\s\*]*?\b(fhip_\w+)\s*\(", text)
    assert len(names) == 5, names
    entries = sorted(n for n in names if n.endswith("_dev"))
    covered = {n for spec in TH.CASES for n in spec.entries}
    assert entries == sorted(covered) == ["fhip_frame_heads_dev", "fhip_gather_frames_dev"]


def test_case_ids_are_unique_and_new():
    ids = [s.id for s in TH.CASES]
    assert len(set(ids)) == len(ids) and not set(ids) & {s.id for s in T.CASES}
    assert {n for s in TH.CASES for n in s.entries} == {"fhip_frame_heads_dev", "fhip_gather_frames_dev"}


@pytest.mark.parametrize("spec", TH.CASES, ids=lambda s: s.id)
def test_poison_versions_differ_in_the_result(oracle, spec):
    case = T.built(spec, oracle)
    assert len(case.sig) == 3 and len(set(case.sig)) == 3, spec.id
    for attr in ("stream", "src"):
        vs = getattr(case, attr, None)
        if vs is not None:
            assert len({(a.shape, a.dtype) for a in vs}) == 1, (spec.id, attr)
            assert not any(np.array_equal(vs[i], vs[j]) for i, j in ((0, 1), (0, 2), (1, 2))), (spec.id, attr)


def test_heads_expectation_is_the_format_s(oracle):
    """The heads case's records are what the header parser written from the FLAC format reads out of each version."""
    case = T.built(TH.CASES[0], oracle)
    for v in range(3):
        want = case.want(v)
        for f in range(T.NF_DEC):
            at, size = int(case.off[f]), int(case.fb[f])
            n, vbs, hlen, number = reference((2, 16, 44100, T.N_DEC), bytes(case.stream[v][at:at + size]), size)
            assert (number, n, 1 | (vbs << 1) | (hlen << 8)) == tuple(want[f].tolist())


def test_gather_expectation_accepts_what_the_entry_is_defined_to(oracle):
    case = T.built(TH.CASES[1], oracle)
    for variant in (0, 1):
        dst, fb = case.want(1, variant)
        assert (fb > 0).sum() == 6 and len(dst) == fb.sum() == case.total(variant)
        assert fb.max() == 16385                      # longer than one round of a wave's 16-byte stores
