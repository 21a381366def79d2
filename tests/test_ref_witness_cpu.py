"""oracle/flake_oracle.c held to the reference's own compiled library, frame for frame.  Runs without a GPU.

The witness is oracle/_ref/build/ref_frames: oracle/ref_frames.c linked statically to the libflake_static.a the
reference's own CMake build makes (oracle/Makefile, `refframes`).  For every case of tests/refcases.py the witness's
record -- effective parameters, every flake_encode_frame() call's return value and bytes -- must equal what
fo_set_defaults + the same overrides + Oracle.encode_block give, in a frame buffer of the reference's size
(encode.c:446-453; the three lines of flake_encode_frame's last_frame latch, which fo_encode_block leaves out, stand in
oracle_calls), and the stream must decode to the PCM through oracle/flac_decode.c.

Where the witness is built (a reference tree at build time) every case runs against it live, and live must equal the
record in tests/golden/ref_frames.npz (tests/golden/make_golden.py ref_frames); where no reference build was attempted
the record stands in: call sizes, one SHA-1 per frame, the effective parameters.  `test_which_witness` says which it
was.  A reference tree that left no witness fails (refcases.witness_state), it does not fall back.

The oracle restates no metadata: the header bytes of flake_encode_init, padding_size, validate_params' verdict and the
34 STREAMINFO bytes are held in tests/test_gpu_ref_witness.py, subject against witness."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import oraclelib
import refcases as RC

CASES = RC.cases()
ORACLE_FIELDS = tuple(k for k in RC.PARAM_FIELDS if k not in ("compression", "padding_size"))


@pytest.fixture(scope="module")
def state():
    return RC.witness_state()


@pytest.fixture(scope="module")
def golden():
    return RC.load_golden()


def oracle_params(oracle, c):
    """fo_set_defaults for the case's level, then the same overrides the client applied."""
    fp = oraclelib.FoParams()
    oracle.L.fo_set_defaults(C.byref(fp), c.level)
    fp.channels, fp.sample_rate, fp.bits_per_sample = c.channels, c.rate, c.bps
    for k, v in c.over.items():
        if k != "padding_size":
            setattr(fp, k, v)
    return fp


def frame_buffer_size(fp):
    """encode.c:446-453: the frame buffer is 3/2 of the largest frame a full block may take before it is re-encoded
    verbatim."""
    if fp.channels == 2:
        mfs = 16 + ((fp.block_size * (2 * fp.bits_per_sample + 1) + 7) >> 3)
    else:
        mfs = 16 + ((fp.block_size * fp.channels * fp.bits_per_sample + 7) >> 3)
    return mfs * 3 // 2


def oracle_calls(oracle, c, pcm, first_count=0, order=None):
    """[(block size, return value, bytes)] of Oracle.encode_block over the case's calls.  first_count and order serve
    the discrimination checks: a frame counter that starts elsewhere, blocks taken in another order."""
    fp = oracle_params(oracle, c)
    buf = frame_buffer_size(fp)
    starts = np.concatenate([[0], np.cumsum(c.blocks)])
    out, fc, last_frame = [], first_count, False
    for i in (range(len(c.blocks)) if order is None else order):
        n = c.blocks[i]
        if last_frame:                                  # encode.c:991-992: nothing follows the short block
            out.append((n, -1, b""))
            continue
        last_frame = not fp.allow_vbs and n != fp.block_size          # encode.c:993-994, which fo_encode_block leaves out
        rc, data, fc = oracle.encode_block(fp, fc, pcm[starts[i]:starts[i] + n], n, buf)
        out.append((n, rc, data.tobytes()))
    return out


def recorded_calls_difference(calls, exp, streaminfo):
    """The oracle's calls against a golden entry (sizes and one SHA-1 per frame): None, or the first difference."""
    if [n for n, _, _ in calls] != [int(x) for x in exp["call_n"]]:
        return "the calls' block sizes differ from the recorded ones"
    f = 0
    for i, (n, rc, data) in enumerate(calls):
        if rc != int(exp["call_ret"][i]):
            return f"call {i} (block of {n}): returned {rc}, the witness recorded {int(exp['call_ret'][i])}"
        frames = RC.split_frames(data, streaminfo) if rc > 0 else []
        if len(frames) != int(exp["call_frames"][i]):
            return f"call {i}: {len(frames)} frames, the witness recorded {int(exp['call_frames'][i])}"
        for k, fr in enumerate(frames):
            if hashlib.sha1(fr).digest() != exp["frame_sha"][f].tobytes():
                return f"call {i}, frame {k} (frame {f} of the stream) has other bytes than the witness recorded: [{RC.describe(fr)}]"
            f += 1
    return None


def test_which_witness(state):
    print(f"\nreference witness: {state} ({RC.WITNESS if state == 'live' else RC.GOLDEN})")
    assert state in ("live", "recorded")


def test_table_is_admissible_and_complete():
    """Exclusions are predicates on the table: every case may only produce frames the reference defines, the random
    family keeps the narrower rule it was drawn under, and no family is empty."""
    for c in CASES:
        assert RC.admissible(c) is None, (c.name, RC.admissible(c))
        if c.family == "random":
            assert RC.strictly_admissible(c) is None, (c.name, RC.strictly_admissible(c))
    by_family = {f: sum(c.family == f for c in CASES) for f in RC.FAMILIES}
    assert all(by_family.values()), by_family
    assert by_family["random"] >= 500
    assert len([c for c in CASES if c.shipped]) >= 8
    # the predicates themselves: each refuses what it is there for
    assert RC.admissible(RC.Case("x", "blocks", 5, "tone", tail=255, block_size=1024)) is not None       # odd LPC tail
    assert RC.admissible(RC.Case("x", "blocks", 8, "tone", tail=12, block_size=1024)) is not None        # 12 <= order 12
    assert RC.admissible(RC.Case("x", "blocks", 9, "tone", tail=0, block_size=136)) is not None          # eighths of 17
    assert RC.admissible(RC.Case("x", "formats", 5, "tone", 2, 32, block_size=1024)) is not None         # 33-bit side
    assert RC.admissible(RC.Case("x", "formats", 5, "tone", 2, 32, block_size=1024, stereo_method=0)) is None
    assert RC.admissible(RC.Case("x", "blocks", 2, "tone", tail=255, block_size=1024)) is None           # fixed: any length


def test_golden_covers_the_table(golden):
    assert sorted(golden) == sorted(c.name for c in CASES)
    nframes = sum(len(e["frame_sha"]) for e in golden.values())
    print(f"\n{len(golden)} cases, {nframes} frames recorded")


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_oracle_equals_witness(oracle, decoder, state, golden, c):
    pcm = c.pcm()
    exp = golden[c.name]
    assert RC.pcm_sha1(pcm) == exp["pcmsha"].tobytes(), \
        f"{c.name}: the generated PCM is not the PCM the record was made from (a drift in generation, not in parity)"
    if state == "live":
        rec = RC.run_client(RC.WITNESS, c, pcm)
        diff = RC.entry_difference(RC.golden_entry(c, rec, pcm), exp)
        assert diff is None, f"{c.name}: the live witness differs from tests/golden/ref_frames.npz: {diff}"
        params, streaminfo = rec.params, rec.streaminfo
        assert rec.valid >= 0 and rec.header_len > 0 and rec.si_rc == 0
    else:
        params = {k: int(v) for k, v in zip(RC.PARAM_FIELDS, exp["params"])}
        streaminfo = exp["streaminfo"].tobytes()
        assert exp["valid"] >= 0 and exp["si_rc"] == 0

    fp = oracle_params(oracle, c)
    for k in ORACLE_FIELDS:
        assert getattr(fp, k) == params[k], f"{c.name}: effective {k}: oracle {getattr(fp, k)}, witness {params[k]}"
    assert params["compression"] == c.level

    calls = oracle_calls(oracle, c, pcm)
    if state == "live":
        diff = RC.first_difference(calls, rec.calls, streaminfo, what=("oracle", "witness"))
    else:
        diff = recorded_calls_difference(calls, exp, streaminfo)
    assert diff is None, f"{c.name}: {diff}"
    refused = RC.REFUSED_CALLS.get(c.name, [])
    assert all((rc == -1) if i in refused else (rc > 0) for i, (_, rc, _) in enumerate(calls)), c.name

    stream = b"".join(b for _, _, b in calls)
    encoded = sum(n for n, rc, _ in calls if rc > 0)            # the refused calls' samples are behind the others
    out, sizes = decoder.decode(np.frombuffer(stream, np.uint8), c.channels, c.bps, c.total)
    assert out.shape[0] == encoded and (out == pcm[:encoded]).all(), f"{c.name}: the stream does not decode to the PCM"
    assert len(sizes) == int(exp["call_frames"].sum()), f"{c.name}: frame count"


# ---- discrimination: the comparison must fail when the oracle is asked for something else ---------------------------

def witness_calls(state, golden, c, pcm):
    """(calls or None, entry, streaminfo): the live calls where there are any."""
    exp = golden[c.name]
    if state == "live":
        rec = RC.run_client(RC.WITNESS, c, pcm)
        return rec.calls, exp, rec.streaminfo
    return None, exp, exp["streaminfo"].tobytes()


def difference(calls, wcalls, exp, streaminfo):
    if wcalls is not None:
        return RC.first_difference(calls, wcalls, streaminfo, what=("oracle", "witness"))
    return recorded_calls_difference(calls, exp, streaminfo)


def test_max_order_7_is_not_max_order_8(oracle, state, golden):
    """lpc_max_1_8, call 0, frame 0: the witness's frame at max order 8 (order method MAX: every LPC subframe has order
    8) is not the oracle's at max order 7."""
    c = RC.case("lpc_max_1_8")
    pcm = c.pcm()
    wcalls, exp, si = witness_calls(state, golden, c, pcm)
    other = RC.Case("lpc_max_1_7", "orders", c.level, c.signal, tail=256, seed=c.seed,
                    **dict(c.over, max_prediction_order=7))
    assert other.blocks == c.blocks
    diff = difference(oracle_calls(oracle, other, pcm), wcalls, exp, si)
    assert diff is not None and diff.startswith("call 0"), diff
    assert difference(oracle_calls(oracle, c, pcm), wcalls, exp, si) is None


def test_frame_counter_off_by_one_fails(oracle, state, golden):
    """level5_tone, call 0, frame 0: the same frames numbered from 1 carry another header and CRCs."""
    c = RC.case("level5_tone")
    pcm = c.pcm()
    wcalls, exp, si = witness_calls(state, golden, c, pcm)
    calls = oracle_calls(oracle, c, pcm, first_count=1)
    diff = difference(calls, wcalls, exp, si)
    assert diff is not None and diff.startswith("call 0"), diff
    assert [rc for _, rc, _ in calls] == [int(x) for x in exp["call_ret"]]        # only the number differs: sizes stay


def test_swapped_blocks_fail(oracle, state, golden):
    """level5_transient, call 0, frame 0: blocks 0 and 1 taken in swapped order."""
    c = RC.case("level5_transient")
    pcm = c.pcm()
    wcalls, exp, si = witness_calls(state, golden, c, pcm)
    diff = difference(oracle_calls(oracle, c, pcm, order=[1, 0, 2, 3]), wcalls, exp, si)
    assert diff is not None and diff.startswith("call 0"), diff
