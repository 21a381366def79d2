"""A recode set (flake_amd_recode_set_*, flake_amd.RecodeSet): the twelve streams of test_gpu_decode_set.py -- eight with
fixed blocks of 64 at level 5, four with variable block size at level 10 -- go in as FLAC frames, round-robin and in
small device batches, and come out re-encoded at another block size and level.  The contract: every stream's output is
byte for byte what a StreamSet at the same parameters writes for that stream's original PCM (whole blocks, then the
tail), its STREAMINFO included, the digest being the one the decode side computed.  Every comparison is exact."""
import math

import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_decode_set import BATCH, as_call, encode_set, like_of, round_robin, FIXED_LENS, VBS_LENS

pytestmark = pytest.mark.gpu

V = flake_amd


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(scope="module")
def streams():
    return encode_set(FIXED_LENS, 64, 5, 0, 100) + encode_set(VBS_LENS, 256, 10, V.SET_VBS, 200)


def reference(pcms, bs, level, flags):
    """What a StreamSet writes for these streams: [(frame bytes, the 34 STREAMINFO bytes, bytes of the whole blocks)]."""
    S = len(pcms)
    whole, tail = [b""] * S, [b""] * S
    with V.StreamSet(S, level=level, flags=flags, block_size=bs) as st:
        blocks = sorted((j, s) for s in range(S) for j in range(len(pcms[s]) // bs))
        if blocks:
            out, sizes = st.encode(np.concatenate([pcms[s][j * bs:(j + 1) * bs] for j, s in blocks]), bs, [s for _, s in blocks])
            at = 0
            for (j, s), n in zip(blocks, sizes):
                whole[s] += out[at:at + n].tobytes()
                at += n
        tails = [(s, len(pcms[s]) % bs) for s in range(S) if len(pcms[s]) % bs]
        if tails:
            out, sizes = st.encode_ragged(np.concatenate([pcms[s][len(pcms[s]) - t:] for s, t in tails]), [t for _, t in tails],
                                          [s for s, _ in tails])
            at = 0
            for (s, t), n in zip(tails, sizes):
                tail[s] = out[at:at + n].tobytes()
                at += n
        return [(whole[s] + tail[s], st.streaminfo_bytes(s), whole[s]) for s in range(S)]


CASES = {"96 at level 8": (96, 8, 0), "64 at level 8": (64, 8, 0), "160 at level 10": (160, 10, V.SET_VBS)}
_refs = {}


def ref_for(streams, case):
    if case not in _refs:
        bs, level, flags = CASES[case]
        _refs[case] = reference([x["pcm"] for x in streams], bs, level, flags)
    return _refs[case]


def refused(rs, call, **kw):
    before = rs.device_batches()
    with pytest.raises(V.FlakeHipError):
        rs.recode_runs(call, **kw)
    assert rs.device_batches() == before
    return rs.last_error()


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_twelve_streams_recoded_byte_for_byte(streams, monkeypatch, case, verify):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    bs, level, flags = CASES[case]
    want = ref_for(streams, case)
    runs = round_robin(streams, 3)
    calls = [runs[c0:c0 + 9] for c0 in range(0, len(runs), 9)]
    assert len(calls) >= 3
    got = [b""] * len(streams)
    with V.RecodeSet(like_of(streams), len(streams), level=level, flags=flags, block_size=bs) as rs:
        rs.set_verify(verify)
        want_dec = 0
        for i, call in enumerate(calls):
            args = as_call(streams, call)
            nframes = sum(n for _, _, n in call)
            need_bytes, need_blocks = rs.out_bound(nframes)
            if i == 1:
                # bad arguments change nothing: room below the bound, a stream outside the set, sizes past the bytes
                assert need_blocks > 0
                assert "bound" in refused(rs, args, out_size=need_bytes - 1)
                assert "bound" in refused(rs, args, block_cap=need_blocks - 1)
                assert "outside" in refused(rs, [(len(streams), args[0][1], args[0][2])] + args[1:])
                refused(rs, [(args[0][0], args[0][1][:-3], args[0][2])])
            for s, data in rs.recode_runs(args):
                got[s] += data
            want_dec += math.ceil(nframes / BATCH)
        dec, enc = rs.device_batches()
        assert dec == want_dec                                      # not one per stream or per run
        for s in range(len(streams)):
            assert got[s] == want[s][2], (s, len(got[s]), len(want[s][2]))          # the whole blocks so far
        ntails = sum(1 for x in streams if len(x["pcm"]) % bs)
        assert rs.out_bound(-1)[1] == ntails
        for s, data in rs.finish():
            got[s] += data
        assert rs.device_batches() == (dec, enc + math.ceil(ntails / BATCH))          # not one per stream
        for s, x in enumerate(streams):
            assert got[s] == want[s][0], s
            assert rs.streaminfo_bytes(s) == want[s][1], s
            assert bytes(rs.streaminfo(s).md5sum) == bytes(x["si"].md5sum), s
            assert rs.failed(s) is None
        # the set takes no more frames
        assert "finished" in refused(rs, as_call(streams, calls[0]))
        with pytest.raises(V.FlakeHipError):
            rs.finish()
    if case.startswith("64"):
        assert ntails == sum(1 for n in FIXED_LENS + VBS_LENS if n % 64) < len(streams)      # some streams have no tail


def test_one_flipped_bit_fails_one_stream(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    want = ref_for(streams, "96 at level 8")
    victim, vf = 2, 4
    x = streams[victim]
    bad = x["frames"].copy()
    bad[x["off"][vf] + x["sizes"][vf] // 2] ^= 0x08
    frames = [y["frames"] for y in streams]
    frames[victim] = bad
    with V.DecodeSet(like_of(streams), len(streams)) as ds:         # what the decode set says of the same call
        ds.decode_runs(as_call(streams, round_robin(streams, 3), frames), sum(len(y["pcm"]) for y in streams))
        verdict = ds.failed(victim)
    assert verdict is not None and verdict[0] == vf
    got = [b""] * len(streams)
    with V.RecodeSet(like_of(streams), len(streams), level=8, block_size=96) as rs:
        for s, data in rs.recode_runs(as_call(streams, round_robin(streams, 3), frames)):
            got[s] += data
        assert rs.failed(victim) == verdict
        # the run before the failing one stands: frames 0 .. 2 are 192 samples, two blocks of 96
        two = got[victim]
        assert two and want[victim][2].startswith(two)
        fs, used = V.index_frames(V.read_streaminfo(want[victim][1])[0], np.frombuffer(two, np.uint8))
        assert len(fs) == 2 and used == len(two)
        # a later call that names the failed stream is refused whole
        assert "failed" in refused(rs, as_call(streams, [(0, 0, 1), (victim, 0, 1)], frames))
        tails = dict(rs.finish())
        assert victim not in tails                                   # no tail
        for s, data in tails.items():
            got[s] += data
        assert rs.streaminfo(victim) is None and rs.streaminfo_bytes(victim) is None
        assert got[victim] == two
        for s in range(len(streams)):
            if s != victim:
                assert got[s] == want[s][0] and rs.streaminfo_bytes(s) == want[s][1] and rs.failed(s) is None, s


def test_md5_off_leaves_the_digest_zero(streams, monkeypatch):
    want = ref_for(streams, "96 at level 8")
    with V.RecodeSet(like_of(streams), 1, level=8, flags=V.SET_MD5_OFF, block_size=96) as rs:
        x = streams[3]
        got = b"".join(d for _, d in rs.recode_runs([(0, x["frames"], x["sizes"])]) + rs.finish())
        assert got == want[3][0]
        assert rs.streaminfo_bytes(0) == want[3][1][:18] + bytes(16)


def test_open_time_refusals(streams):
    like = like_of(streams)
    for kw, text in ((dict(flags=V.SET_MD5_HOST), "MD5_HOST"), (dict(bits_per_sample=24), "source format"),
                     (dict(channels=1), "source format"), (dict(level=10), "variable block size"),
                     (dict(level=5, flags=V.SET_VBS), "FLAKE_AMD_SET_VBS needs")):
        with pytest.raises(V.FlakeHipError) as e:
            V.RecodeSet(like, 2, **kw)
        assert text in str(e.value), (kw, str(e.value))
