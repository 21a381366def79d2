"""The HIP frames held to the reference's own compiled library.

tests/golden/ref_frames.npz is what the witness (oracle/_ref/build/ref_frames: oracle/ref_frames.c on the reference's
own libflake_static.a) answered to every case of tests/refcases.py; tests/test_ref_witness_cpu.py holds the record to
the live witness wherever a reference tree is.  Here the subject is the shipped drop-in, libflake.so -> host layer ->
K0..K4, on two legs:

  in process   flake_amd.HostEncoder on every case outside the random family, one block per flake_encode_frame() call
               as the witness made them: every return value, one SHA-1 per frame, the final 34 STREAMINFO bytes and
               the header of flake_encode_init() against the record;
  as shipped   the same client source linked to libflake.so (oracle/_ref/ref_frames_hip on the reference's flake.h, or
               oracle/ref_frames_own on this project's header where no reference tree was at build time) as a fresh
               child process per case, its whole record against the witness's -- the live witness where it travelled,
               else the record -- and two cases again under FLAKE_AMD_LOOKAHEAD=8.

Two metadata fields may differ and are named in refcases.METADATA_ALLOWED (the vendor string; the MD5 field of the
provisional STREAMINFO in flake_encode_init()'s header); anything else unequal fails.  The coverage conditions at the
end are computed from the witness's recorded frames (one feature word per frame, read from the witness's bytes with
flake_amd.index_frames and the frame parser of tests/test_format_edges_cpu.py): the subset of cases that runs here
cannot go soft without a test failing."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import flake_amd
import refcases as RC

pytestmark = pytest.mark.gpu

GPU_CASES = RC.gpu_cases()
SHIPPED = [c for c in GPU_CASES if c.shipped]
LOOKAHEAD = ["level10_transient", "frames_130_mono"]
CHILD_TIMEOUT = 60          # a context start and a few frames


@pytest.fixture(scope="module")
def golden():
    return RC.load_golden()


def subject_program():
    for exe in (RC.SUBJECT, os.path.join(RC.ROOT, "oracle", "ref_frames_own")):
        if os.path.exists(exe):
            return exe
    raise FileNotFoundError("oracle/ref_frames_own is not built: run build()")


def header_ok(got: bytes, exp: bytes, what):
    diffs = RC.metadata_differences(got, exp, streaminfo=False)
    assert set(diffs) <= set(RC.METADATA_ALLOWED), f"{what}: the header of flake_encode_init() differs in {diffs}"


@pytest.mark.parametrize("c", GPU_CASES, ids=lambda c: c.name)
def test_in_process(golden, c):
    exp = golden[c.name]
    pcm = c.pcm()
    assert RC.pcm_sha1(pcm) == exp["pcmsha"].tobytes(), f"{c.name}: the generated PCM is not the recorded one"
    si34 = exp["streaminfo"].tobytes()
    starts = np.concatenate([[0], np.cumsum(c.blocks)])
    with flake_amd.HostEncoder(c.level, c.channels, c.bps, c.rate, c.samples, **c.over) as enc:
        got = {k: getattr(enc.ctx.params, k) for k in RC.PARAM_FIELDS}
        want = {k: int(v) for k, v in zip(RC.PARAM_FIELDS, exp["params"])}
        assert got == want, f"{c.name}: effective parameters"
        assert enc.subset == exp["valid"], f"{c.name}: validate_params {enc.subset}, witness {exp['valid']}"
        header_ok(enc.header, exp["header"].tobytes(), c.name)
        f = 0
        for i, n in enumerate(c.blocks):
            if int(exp["call_ret"][i]) < 0:                    # a call the reference refuses (refcases.REFUSED_CALLS)
                assert i in RC.REFUSED_CALLS[c.name]
                with pytest.raises(flake_amd.FlakeHipError) as err:
                    enc.encode_frame(pcm[starts[i]:starts[i] + n])
                assert err.value.code == int(exp["call_ret"][i]), f"{c.name}: call {i} returned {err.value.code}"
                continue
            data = enc.encode_frame(pcm[starts[i]:starts[i] + n])
            assert len(data) == int(exp["call_ret"][i]), \
                f"{c.name}: call {i} (block of {n}) returned {len(data)}, the witness {int(exp['call_ret'][i])}"
            frames = RC.split_frames(data, si34)
            assert len(frames) == int(exp["call_frames"][i]), f"{c.name}: call {i}: {len(frames)} frames"
            for k, fr in enumerate(frames):
                assert hashlib.sha1(fr).digest() == exp["frame_sha"][f].tobytes(), \
                    f"{c.name}: call {i}, frame {k} (frame {f} of the stream) is not the witness's: [{RC.describe(fr)}]"
                f += 1
        assert f == len(exp["frame_sha"])
        assert flake_amd.write_streaminfo(enc.streaminfo()) == si34, f"{c.name}: STREAMINFO"


def shipped_run(golden, c, tmp_env=None):
    """The subject's record of this case from a fresh child process, against the witness's."""
    pcm = c.pcm()
    exp = golden[c.name]
    env = dict(os.environ, **(tmp_env or {}))
    got = RC.run_client(subject_program(), c, pcm, env=env, timeout=CHILD_TIMEOUT)
    if os.path.exists(RC.WITNESS):
        wit = RC.run_client(RC.WITNESS, c, pcm, timeout=CHILD_TIMEOUT)
        used = "the live witness"
        assert RC.entry_difference(RC.golden_entry(c, wit, pcm), exp) is None, f"{c.name}: live witness against its record"
        diff = RC.first_difference(got.calls, wit.calls, wit.streaminfo, what=("subject", "witness"))
        assert diff is None, f"{c.name}: {diff}"
        assert (got.valid, got.params, got.si_rc, got.streaminfo) == (wit.valid, wit.params, wit.si_rc, wit.streaminfo), c.name
        header_ok(got.header, wit.header, c.name)
    else:
        used = "the witness's record"
    entry = RC.golden_entry(c, got, pcm)
    header_ok(got.header, exp["header"].tobytes(), c.name)
    entry["header"] = exp["header"]
    diff = RC.entry_difference(entry, exp)
    assert diff is None, f"{c.name}: subject against {used}: {diff}"
    print(f"\n{c.name}: {os.path.basename(subject_program())} against {used}: {len(entry['frame_sha'])} frames equal")


@pytest.mark.parametrize("c", SHIPPED, ids=lambda c: c.name)
def test_as_shipped(golden, c):
    shipped_run(golden, c)


@pytest.mark.parametrize("name", LOOKAHEAD)
def test_as_shipped_lookahead(golden, name):
    """FLAKE_AMD_LOOKAHEAD=8 queues whole blocks behind the same calls; the sum of what the calls return and the
    stream they leave are the witness's, though a call may return 0 and a later one several blocks' frames."""
    c = RC.case(name)
    assert c.samples_known          # the queue needs the stream's length
    pcm = c.pcm()
    exp = golden[c.name]
    got = RC.run_client(subject_program(), c, pcm, env=dict(os.environ, FLAKE_AMD_LOOKAHEAD="8"), timeout=CHILD_TIMEOUT)
    assert all(rc >= 0 for _, rc, _ in got.calls), [rc for _, rc, _ in got.calls]
    stream = b"".join(b for _, _, b in got.calls)
    assert len(stream) == int(exp["call_ret"].sum())
    frames = RC.split_frames(stream, exp["streaminfo"].tobytes())
    assert len(frames) == len(exp["frame_sha"])
    for f, fr in enumerate(frames):
        assert hashlib.sha1(fr).digest() == exp["frame_sha"][f].tobytes(), f"{name}: frame {f}: [{RC.describe(fr)}]"
    assert got.streaminfo == exp["streaminfo"].tobytes() and got.si_rc == 0
    header_ok(got.header, exp["header"].tobytes(), name)


def test_shipped_cases_are_the_ones_asked_for():
    names = {c.name for c in SHIPPED}
    assert names == {"level5_transient", "level10_transient", "format_8ch_16bit_level5", "format_1ch_24bit_level8",
                     "rate_12345", "frames_130_mono", "level3_noise", "samples_unknown"}


# ---- coverage: what the cases of this file contain, by the witness's recorded frames ---------------------------------

@pytest.fixture(scope="module")
def feats(golden):
    return {c.name: golden[c.name]["frame_feat"] for c in GPU_CASES}


def test_coverage_of_the_gpu_cases(golden, feats):
    all_f = np.concatenate(list(feats.values()))
    assert len(all_f) == sum(len(golden[c.name]["frame_sha"]) for c in GPU_CASES)
    ch = set(all_f["ch_code"].tolist())
    assert {1, 8, 9, 10} <= ch, f"channel assignments {sorted(ch)}"                 # independent, L/S, R/S, M/S
    sub = int(np.bitwise_or.reduce(all_f["subframes"]))
    for bit, name in ((RC.F_CONSTANT, "CONSTANT"), (RC.F_VERBATIM, "VERBATIM"), (RC.F_FIXED, "FIXED"), (RC.F_LPC, "LPC"),
                      (RC.F_WASTED, "a wasted-bits flag")):
        assert sub & bit, f"no frame with {name}"
    # a verbatim re-encoded frame: optimize.c:154 chooses VERBATIM itself only below 5 samples or without prediction
    reenc = [c.name for c in GPU_CASES if c.setting("prediction_type") != RC.PRED_NONE
             and ((feats[c.name]["subframes"] & RC.F_VERBATIM != 0) & (feats[c.name]["n"] >= 5)).any()]
    assert reenc, "no frame re-encoded verbatim"
    # variable block size: a block split into several frames, and one left whole
    vbs = [golden[c.name]["call_frames"] for c in GPU_CASES if c.setting("variable_block_size")]
    assert any((v > 1).any() for v in vbs) and any((v == 1).any() for v in vbs)
    bs = set(all_f["bs_code"].tolist())
    assert bs & {1, 2, 3, 4, 5} and bs & set(range(8, 16)) and {6, 7} <= bs, f"block-size codes {sorted(bs)}"
    sr = set(all_f["sr_code"].tolist())
    assert sr & set(range(4, 12)) and {12, 13, 14} <= sr, f"sample-rate codes {sorted(sr)}"
    fixed_nb = set(all_f["number_bytes"][all_f["vbs"] == 0].tolist())
    var_nb = set(all_f["number_bytes"][all_f["vbs"] == 1].tolist())
    assert 2 in fixed_nb, "no 2-byte frame number"
    assert 3 in var_nb and 4 in var_nb, "no 3-byte sample number, or none past 2^16"
    # the as-shipped subset on its own
    ship = np.concatenate([feats[c.name] for c in SHIPPED])
    ssub = int(np.bitwise_or.reduce(ship["subframes"]))
    assert ssub & RC.F_VERBATIM and ssub & RC.F_LPC and 13 in ship["sr_code"] and 2 in ship["number_bytes"]
    assert (golden["level10_transient"]["call_frames"] > 1).any()


# ---- the command-line tools, whole files -----------------------------------------------------------------------------

def write_wav(path, pcm16, rate):
    raw = pcm16.astype("<i2").tobytes()
    ch = pcm16.shape[1]
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * 2 * ch, 2 * ch, 16) + b"data" +
                struct.pack("<I", len(raw)) + raw)


@pytest.mark.parametrize("level", [5, 10])
def test_cli_file_equals_the_reference_cli(tmp_path, level):
    """The reference's own `flake` (oracle/_ref/build/flake, its CMake build) and flake_amd_cli on one small WAV: the
    frames from the first sync on and the STREAMINFO block are equal; of the other metadata only what
    refcases.METADATA_ALLOWED names may differ."""
    ref_cli = os.path.join(RC.REF_DIR, "build", "flake")
    if not os.path.exists(ref_cli):
        pytest.skip("the reference's flake program did not travel here (no reference tree at build time), and whole "
                    "files have no record")
    c = RC.case("level10_transient")
    wav = tmp_path / "in.wav"
    write_wav(wav, c.pcm(), 44100)
    outs = []
    for exe, args in ((ref_cli, [f"-{level}", str(wav), "-o", str(tmp_path / "ref.flac")]),
                      (os.path.join(flake_amd.LIB_DIR, "flake_amd_cli"), [f"-{level}", str(wav), str(tmp_path / "hip.flac")])):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, r.stderr + r.stdout
        with open(args[-1], "rb") as f:
            outs.append(f.read())
    ref, hip = outs
    diffs = RC.metadata_differences(hip, ref)
    assert set(diffs) <= {"vendor string"}, f"metadata differs in {diffs}"
    (_, rend), (_, hend) = RC.metadata_blocks(ref), RC.metadata_blocks(hip)
    assert ref[rend:rend + 2] in (b"\xff\xf8", b"\xff\xf9")
    assert hip[hend:] == ref[rend:], "audio frames differ"
    assert len(ref) - rend > 1000
