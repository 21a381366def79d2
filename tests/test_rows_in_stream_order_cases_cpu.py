"""The CPU side of tests/test_gpu_rows_in_stream_order.py: every *_dev entry of include/flakehip_rows_in.h has its case
there, and the case's poison conditions hold -- the witness gives three pairwise different results for versions A, B and
C of one geometry, so that work which saw the wrong version cannot pass -- and the witness is what the header's rule
says on values whose answer is known, not what the entry gives."""
import os
import re

import numpy as np
import pytest

import test_gpu_rows_in_stream_order as TR
import test_gpu_stream_order as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_device_entry_of_the_rows_in_header_has_a_case():
    """tests/test_stream_order_cases_cpu.py holds include/flakehip.h's device entries to the cases of
    tests/test_gpu_stream_order.py; the encode-rows entries are declared in include/flakehip_rows_in.h and have their
    cases in tests/test_gpu_rows_in_stream_order.py: the same condition, on that pair.  fhip_frames_packed_from_rows
    synchronises before it returns."""
    text = open(os.path.join(ROOT, "include", "flakehip_rows_in.h")).read()
    names = re.findall(r"FHIP_API\s+[\w\s\*]*?\b(fhip_\w+)\s*\(", text)
    assert sorted(names) == ["fhip_frames_packed_from_rows", "fhip_pcm_from_rows_dev"], names
    entries = sorted(n for n in names if n.endswith("_dev"))
    covered = {n for spec in TR.CASES for n in spec.entries}
    assert entries == sorted(covered) == ["fhip_pcm_from_rows_dev"]


def test_case_ids_are_unique_and_new():
    ids = [s.id for s in TR.CASES]
    assert len(set(ids)) == len(ids) and not set(ids) & {s.id for s in T.CASES}


@pytest.mark.parametrize("spec", TR.CASES, ids=lambda s: s.id)
def test_poison_versions_differ_in_the_result(oracle, spec):
    case = T.built(spec, oracle)
    assert len(case.sig) == 3 and len(set(case.sig)) == 3, spec.id
    vs = case.src
    assert len({(a.shape, a.dtype) for a in vs}) == 1
    assert not any(np.array_equal(vs[i], vs[j]) for i, j in ((0, 1), (0, 2), (1, 2)))
    for variant in (0, 1):
        want = case.want(1, variant)
        assert want.shape == (TR.ROWS_IN_TOTAL, 2) and want.dtype == np.int32


def test_the_witness_is_the_header_s_rule():
    e = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1.5 / 32768, 2.5 / 32768, -1.5 / 32768, -2.5 / 32768, np.nan, np.inf, -np.inf,
                  np.nextafter(np.float32(1), np.float32(0))], np.float32)
    assert TR.rows_in_conv(e, 16).tolist() == [0, 0, 32767, -32768, 16384, 2, 2, -2, -2, 0, 32767, -32768, 32767]
    assert TR.rows_in_conv(np.array([1.0, -1.0, 0.99999994], np.float32), 32).tolist() == [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 128]
