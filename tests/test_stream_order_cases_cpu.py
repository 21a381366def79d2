"""Completeness of tests/test_gpu_stream_order.py, on the CPU: every device entry of include/flakehip.h has an ordering
case or a written reason for having none, and every case's poison conditions hold -- the witness gives three pairwise
different results for versions A, B and C, so that work which saw the wrong version cannot pass."""
import os
import re

import numpy as np
import pytest

import flake_amd
import test_gpu_stream_order as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entries that are not named *_dev but run device work on a stream of the handle's own beside the caller's
ALSO = ["fhip_frames_packed_fetch_async", "fhip_frames_packed_gather", "fhip_md5_update_uploaded",
        "fhip_md5_update_uploaded_ragged"]


def device_entries():
    text = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    names = re.findall(r"FHIP_API\s+[\w\s\*]*?\b(fhip_\w+)\s*\(", text)
    assert len(names) > 60 and "fhip_create" in names, names
    return sorted({n for n in names if n.endswith("_dev")} | set(ALSO))


def test_every_device_entry_has_a_case_or_a_reason():
    entries = device_entries()
    assert len([n for n in entries if n.endswith("_dev")]) >= 18, entries
    for n in ALSO:
        assert re.search(r"FHIP_API[^;]*\b%s\s*\(" % n, open(os.path.join(ROOT, "include", "flakehip.h")).read()), n
    covered = {n for spec in T.CASES for n in spec.entries} | set(T.SEQUENCE_ENTRIES)
    for name, test in T.SEQUENCE_ENTRIES.items():
        assert callable(getattr(T, test)), (name, test)
    missing = [n for n in entries if n not in covered and n not in T.EXCLUDED]
    assert not missing, f"device entries with neither an ordering case nor a reason in EXCLUDED: {missing}"
    for n, why in T.EXCLUDED.items():
        assert n in entries, f"EXCLUDED names {n}, which the header does not declare"
        assert n not in covered, f"{n} is covered and excluded"
        assert isinstance(why, str) and len(why.split()) >= 5, (n, why)
    unknown = sorted(covered - set(entries))
    assert not unknown, f"cases name entries the header does not declare: {unknown}"
    print("\n".join(f"{n}: {'covered' if n in covered else 'excluded -- ' + T.EXCLUDED[n]}" for n in entries))


def test_case_ids_are_unique():
    ids = [s.id for s in T.CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("spec", T.CASES, ids=lambda s: s.id)
def test_poison_versions_differ_in_the_result(oracle, spec):
    """expected(A), expected(B) and expected(C) are pairwise different, and the three versions of every bulk input
    have one geometry."""
    case = T.built(spec, oracle)
    assert len(case.sig) == 3 and len(set(case.sig)) == 3, spec.id
    for attr in ("pcm", "stream", "src"):
        vs = getattr(case, attr, None)
        if vs is not None:
            flat = [np.concatenate([np.ravel(a) for a in v]) if isinstance(v, list) else np.ravel(v) for v in vs]
            assert len({(a.shape, a.dtype) for a in flat}) == 1, (spec.id, attr)
            assert not any(np.array_equal(flat[i], flat[j]) for i, j in ((0, 1), (0, 2), (1, 2))), (spec.id, attr)


def test_index_expectation_is_the_cpu_indexer_s(oracle):
    """The index case's table is flacgen's frame table cut where a broken CRC-16 stops the walk; the CPU indexer, whose
    answer the device entry is defined to give, says the same for every version and range."""
    spec = next(s for s in T.CASES if s.id == "index_ranges")
    case = T.built(spec, oracle)
    si = flake_amd.HostStreaminfo(min_block_size=T.N_DEC, max_block_size=T.N_DEC, sample_rate=44100, channels=2,
                                  bits_per_sample=16)
    rf = case.range_first
    for v in range(3):
        fbytes, found, cons, var = case.want(v)
        at = 0
        for r in range(2):
            sizes, used = flake_amd.index_frames(si, case.stream[v][rf[r]:rf[r + 1]])
            assert len(sizes) == found[r] and used == cons[r], (v, r, len(sizes), used)
            assert sizes.tolist() == fbytes[at:at + found[r]].tolist()
            at += found[r]
        assert (fbytes[at:] == -77).all() and not var.any()


def test_verbatim_streams_decode_to_their_signals(decoder):
    """All three versions of the decode cases' streams are valid FLAC of one frame table: the independent CPU decoder
    gives back each signal."""
    tables = {tuple(T.sizes_of(T.verbatim_frames(s)).tolist()) for s in T.SEEDS}
    assert len(tables) == 1
    for s in T.SEEDS:
        out, bs = decoder.decode(T.as_u8(T.verbatim_frames(s)), 2, 16, T.N_DEC * T.NF_DEC)
        assert np.array_equal(out, T.signal(s)) and bs.tolist() == [T.N_DEC] * T.NF_DEC
    out, _ = decoder.decode(T.as_u8(T.verbatim_frames(T.SEEDS[1], True)), 2, 16, T.N_DEC * T.NF_DEC)
    assert np.array_equal(out, T.signal(T.SEEDS[1]))
