"""The set layer (flake_amd_decode_set_*, flake_amd_decode_set_windows, flake_amd_recode_set_*) beyond stereo 16-bit
streams of tiny blocks: tests/setcases.py's families -- F1 formats from (1, 8) to (8, 32), F2 the 1152 / 4608 / 4096
geometries with a stream whose samples never agree with their destination modulo 16 bytes, F3 carries that live for
dozens of steps and seventy streams, F4 frames this encoder never writes, F5 incompressible input at the output bound.
The witnesses are made on the CPU and do not come from the code under test (tests/test_set_cases_cpu.py holds them to the
independent decoder): a decode is held to the PCM the source was made from and to hashlib's digest of it; a recode to the
oracle's flake_encode_frame() loop over that PCM cut at the output block, byte for byte, with the 34 STREAMINFO bytes
worked out from those frames.  Every comparison is exact."""
import hashlib
import math

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
import setcases as sc

pytestmark = pytest.mark.gpu

V = flake_amd
EMPTY_MD5 = hashlib.md5(b"").digest()


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def samples_of(c, call):
    return sum(sum(c["streams"][s]["blocks"][a:a + n]) for s, a, n in call)


# ---- DecodeSet ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.names("F1", "F2", "F4"))
def test_decode_set(name, monkeypatch):
    c = sc.case(name)
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(c["batch"]))
    streams = c["streams"]
    for flags in (0, V.SET_MD5_HOST, V.SET_MD5_OFF):
        for sample_bytes in ((4, 2) if c["bps"] <= 16 else (4,)):
            dt = np.int16 if sample_bytes == 2 else np.int32
            with V.DecodeSet(sc.like_of(c), len(streams), flags) as ds:
                per = [[np.zeros((0, c["ch"]), dt)] for _ in streams]
                for call in c["calls"]:
                    got = ds.decode_runs(sc.as_call(streams, call), samples_of(c, call), sample_bytes)
                    for (s, a, n), part in zip(call, got):
                        assert part is not None and part.dtype == dt, (name, flags, s, a)
                        # (each run where it was cut, so that a mismatch names the run)
                        at = sum(streams[s]["blocks"][:a])
                        assert np.array_equal(part, streams[s]["pcm"][at:at + len(part)].astype(dt)), (name, flags, sample_bytes, s, a)
                        per[s].append(part.copy())
                assert ds.device_batches() == sc.want_decode_batches(c)
                for s, x in enumerate(streams):
                    named = s in c["named"]
                    assert np.array_equal(np.concatenate(per[s]), x["pcm"].astype(dt) if named else x["pcm"][:0]), (name, s)
                    assert ds.failed(s) is None, (name, flags, s, ds.failed(s))
                    if flags & V.SET_MD5_OFF:
                        assert ds.md5(s) is None
                    else:
                        assert ds.md5(s) == (x["md5"] if named else EMPTY_MD5), (name, flags, sample_bytes, s)


# ---- windows of a set -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["F1-1x8", "F1-2x24", "F1-3x24", "F1-6x20"])
def test_decode_windows(name, monkeypatch):
    c = sc.case(name)
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(c["batch"]))
    n = sc.F1_SRC
    wins, want = [], []
    for s in c["named"]:
        x = c["streams"][s]
        total = len(x["pcm"])
        asked = [(skip, take) for skip in (0, n - 1, n, n + 1, total - 1) for take in (1, n, max(total - skip, 0), 0)]
        for skip, take in asked + [(0, total)]:
            wins.append((x["frames"], x["sizes"], n, skip, take))
            want.append(x["pcm"][skip:skip + take])
    for sample_bytes in ((4, 2) if c["bps"] <= 16 else (4,)):
        dt = np.int16 if sample_bytes == 2 else np.int32
        with V.DecodeSet(sc.like_of(c), len(c["streams"]), V.SET_MD5_OFF) as ds:
            res, status, decoded, begins = ds.decode_windows(wins, None, sample_bytes)
            assert list(status) == [0] * len(wins)
            at = 0
            for w, (r, b) in enumerate(zip(res, begins)):
                assert b == at and r.dtype == dt and np.array_equal(r, want[w].astype(dt)), (name, w, wins[w][3:], len(r), len(want[w]))
                at += len(want[w])


# ---- RecodeSet ------------------------------------------------------------------------------------------------------

def refused(rs, call, **kw):
    before = rs.device_batches()
    with pytest.raises(V.FlakeHipError):
        rs.recode_runs(call, **kw)
    assert rs.device_batches() == before
    return rs.last_error()


def decode_again(c, got, exp):
    """The recode's output through a second decode set, every stream in one run: the PCM comes back."""
    runs = [(s, got[s], [f[0] for f in exp[s]["frames"]]) for s in c["named"]]
    like = V.HostStreaminfo(min_block_size=16, max_block_size=c["B"], sample_rate=sc.RATE, channels=c["ch"], bits_per_sample=c["bps"])
    with V.DecodeSet(like, len(c["streams"])) as ds:
        back = ds.decode_runs(runs, sum(len(c["streams"][s]["pcm"]) for s in c["named"]))
        for s, part in zip(c["named"], back):
            assert part is not None and np.array_equal(part, c["streams"][s]["pcm"]), (c["name"], s)
            assert ds.md5(s) == c["streams"][s]["md5"]


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("name", sc.NAMES)
def test_recode_set(name, verify, monkeypatch):
    c = sc.case(name)
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(c["batch"]))
    streams, exp = c["streams"], sc.expected(c)
    S = len(streams)
    got = [b""] * S
    largest = per_block = 0
    with V.RecodeSet(sc.like_of(c), S, level=c["level"], flags=c["flags"], block_size=c["B"]) as rs:
        rs.set_verify(verify)
        for i, call in enumerate(c["calls"]):
            args = sc.as_call(streams, call)
            need_bytes, need_blocks = rs.out_bound(sum(n for _, _, n in call))
            if need_blocks:
                per_block = need_bytes // need_blocks
                assert need_bytes == per_block * need_blocks
                if c["family"] == "F5" or i == 1:
                    assert "bound" in refused(rs, args, out_size=need_bytes - 1)
                    assert "bound" in refused(rs, args, block_cap=need_blocks - 1)
            # exactly at the bound
            for s, data in rs.recode_runs(args, out_size=need_bytes, block_cap=need_blocks):
                got[s] += data
                largest = max(largest, len(data))
        dec, enc = rs.device_batches()
        assert dec == sc.want_decode_batches(c)                     # not one per stream or per run
        for s in range(S):
            assert got[s] == exp[s]["whole"], (name, s, len(got[s]), len(exp[s]["whole"]))      # the whole blocks so far
        ntails = sum(1 for s in c["named"] if len(streams[s]["pcm"]) % c["B"])
        need_bytes, need_blocks = rs.out_bound(-1)
        assert need_blocks == ntails
        if ntails:
            per_block = need_bytes // need_blocks
            with pytest.raises(V.FlakeHipError):
                rs.finish(out_size=need_bytes - 1)
            assert "bound" in rs.last_error() and rs.device_batches() == (dec, enc)
        for s, data in rs.finish(out_size=need_bytes, block_cap=need_blocks):
            got[s] += data
            largest = max(largest, len(data))
        assert rs.device_batches() == (dec, enc + math.ceil(ntails / c["batch"]))      # not one per stream
        for s, x in enumerate(streams):
            assert got[s] == exp[s]["all"], (name, s, len(got[s]), len(exp[s]["all"]))
            assert rs.streaminfo_bytes(s) == exp[s]["si"], (name, s, rs.streaminfo_bytes(s).hex(), exp[s]["si"].hex())
            assert rs.failed(s) is None
            if c["family"] == "F4":
                assert bytes(rs.streaminfo(s).md5sum) == x["si_bytes"][18:]         # the source stream's own
    if c["family"] == "F5":
        # no block takes more than the figure the bound is made of (-s shows both)
        print(f"{name}: largest block {largest} bytes, per-block figure {per_block}, {per_block - largest} to spare")
        assert 0 < largest <= per_block, (name, largest, per_block)
        assert largest == max(b for e in exp for b in e["block_bytes"])
    if not verify:
        decode_again(c, got, exp)


@pytest.mark.parametrize("name", sc.names("F1"))
def test_f1_stream_set_is_a_second_witness(name):
    """What a StreamSet at the same parameters writes for the same PCM (the witness of tests/test_gpu_recode_set.py) is
    the oracle's loop too."""
    c = sc.case(name)
    exp, B = sc.expected(c), c["B"]
    pcms = [c["streams"][s]["pcm"] if s in c["named"] else c["streams"][s]["pcm"][:0] for s in range(len(c["streams"]))]
    S = len(pcms)
    whole, tail = [b""] * S, [b""] * S
    with V.StreamSet(S, level=c["level"], channels=c["ch"], bits_per_sample=c["bps"], flags=c["flags"], block_size=B) as st:
        blocks = sorted((j, s) for s in range(S) for j in range(len(pcms[s]) // B))
        out, sizes = st.encode(np.concatenate([pcms[s][j * B:(j + 1) * B] for j, s in blocks]), B, [s for _, s in blocks])
        at = 0
        for (j, s), n in zip(blocks, sizes):
            whole[s] += out[at:at + n].tobytes()
            at += n
        tails = [(s, len(pcms[s]) % B) for s in range(S) if len(pcms[s]) % B]
        out, sizes = st.encode_ragged(np.concatenate([pcms[s][len(pcms[s]) - t:] for s, t in tails]), [t for _, t in tails],
                                      [s for s, _ in tails])
        at = 0
        for (s, t), n in zip(tails, sizes):
            tail[s] = out[at:at + n].tobytes()
            at += n
        for s in range(S):
            assert whole[s] == exp[s]["whole"] and whole[s] + tail[s] == exp[s]["all"], (name, s)
            assert st.streaminfo_bytes(s) == exp[s]["si"], (name, s)


# ---- one failing stream outside stereo 16 ---------------------------------------------------------------------------

def test_one_flipped_bit_fails_one_stream_of_three_channels(monkeypatch):
    """F1 at (3, 24) to output block 80: a bit in the middle of frame 2 of the longest stream.  Runs of two frames, so
    that the victim's first run (384 samples: four blocks of 80) stands."""
    c = sc.case("F1-3x24")
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(c["batch"]))
    streams, B, victim, vf = c["streams"], 80, 3, 2
    S = len(streams)
    want = [sc.expected_stream(streams[s]["pcm"] if s in c["named"] else streams[s]["pcm"][:0], 3, 24, B, 5, False) for s in range(S)]
    x = streams[victim]
    bad = x["frames"].copy()
    bad[x["off"][vf] + x["sizes"][vf] // 2] ^= 0x08
    frames = [y["frames"] for y in streams]
    frames[victim] = bad
    runs = sc.round_robin(streams, 2, c["named"])
    with V.DecodeSet(sc.like_of(c), S) as ds:                       # what the decode set says of the same call
        parts = ds.decode_runs(sc.as_call(streams, runs, frames), samples_of(c, runs))
        verdict = ds.failed(victim)
        for (s, a, n), part in zip(runs, parts):
            assert (part is None) == (s == victim and a + n > vf)
    assert verdict is not None and verdict[0] == vf
    got = [b""] * S
    with V.RecodeSet(sc.like_of(c), S, level=5, block_size=B) as rs:
        for s, data in rs.recode_runs(sc.as_call(streams, runs, frames)):
            got[s] += data
        assert rs.failed(victim) == verdict
        stood = got[victim]
        assert stood and want[victim]["whole"].startswith(stood)
        fs, used = V.index_frames(V.read_streaminfo(want[victim]["si"])[0], np.frombuffer(stood, np.uint8))
        assert len(fs) == 2 * sc.F1_SRC // B == 4 and used == len(stood)
        assert "failed" in refused(rs, sc.as_call(streams, [(0, 0, 1), (victim, 0, 1)], frames))
        tails = dict(rs.finish())
        assert victim not in tails                                   # no tail
        for s, data in tails.items():
            got[s] += data
        assert rs.streaminfo(victim) is None and rs.streaminfo_bytes(victim) is None
        assert got[victim] == stood
        for s in range(S):
            if s != victim:
                assert got[s] == want[s]["all"] and rs.streaminfo_bytes(s) == want[s]["si"] and rs.failed(s) is None, s
