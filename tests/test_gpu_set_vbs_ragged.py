"""flake_amd_set_encode_ragged on a set with variable block size (FLAKE_AMD_SET_VBS, levels 9-12): the short blocks of
a call -- each of its own length, splittable or not -- run as one device batch per FLAKE_AMD_BATCH of them
(fhip_encode_blocks_vbs_ragged_numbered) instead of one per distinct length.

The yardsticks are the code that already exists: the per-length leg (FLAKE_AMD_SET_RAGGED=0: one flake_amd_set_encode
call per distinct length, the path this entry took before) on a fresh set, a single-stream HostEncoder fed block for
block, hashlib for the MD5 and the test decoder.  The call count is read from flake_amd_set_device_batches."""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import flake_amd
import vbs_ragged_inputs as I

pytestmark = pytest.mark.gpu

V = flake_amd
BS = I.BS
S = 17


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def packed_bytes(pcm, bits):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(pcm.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def tails_for(level):
    """17 distinct tails, all shorter than the block size: the lengths of the ABI test (the full block replaced) and two
    or three more."""
    t = [1136 if n == BS else n for n in I.lengths_for(level)] + [776, 999] + ([888] if level >= 11 else [])
    assert len(t) == S and len(set(t)) == S and max(t) < BS
    return t


def make_streams(level, ch, bits, oracle=None):
    """Stream s: s % 2 whole blocks, then its tail; every block bursts against near-silence per eighth."""
    tails = tails_for(level)
    tail_blocks = I.make_blocks(500 + level, tails, ch, bits)
    if oracle is not None:
        I.oracle_splits(oracle, tail_blocks, ch)
    r = np.random.RandomState(900 + level)
    return [[I.burst_block(r, BS, ch, bits, 1) for _ in range(s % 2)] + [tail_blocks[s]] for s in range(S)]


def open_set(level, ch, bits, flags=0, batch=32):
    with env(FLAKE_AMD_BATCH=batch):
        return V.StreamSet(S, level=level, channels=ch, bits_per_sample=bits, flags=flags | V.SET_VBS, block_size=BS)


def split_frames(got, members, data, sizes):
    pos = 0
    for s, fs in zip(members, sizes):
        got[s] += data[pos:pos + fs].tobytes()
        pos += int(fs)
    assert pos == len(data)


def close_streams(st, streams, ragged, mixed=False):
    """Every stream through the set: the whole blocks in one flake_amd_set_encode call (or, mixed, in the ragged call
    too), the tails in ONE flake_amd_set_encode_ragged call.  Returns the per-stream bytes and by how much
    device_batches() grew over the ragged call."""
    got = [bytearray() for _ in streams]
    items = [(k, s) for s, blocks in enumerate(streams) for k in range(len(blocks))]
    items.sort()                                                 # block k of every stream, then block k + 1
    if not mixed:
        whole = [(k, s) for k, s in items if streams[s][k].shape[0] == BS]
        if whole:
            data, sizes = st.encode(np.concatenate([streams[s][k] for k, s in whole]), BS, [s for _, s in whole])
            split_frames(got, [s for _, s in whole], data, sizes)
        items = [(k, s) for k, s in items if streams[s][k].shape[0] != BS]
    before = st.device_batches()
    with env(FLAKE_AMD_SET_RAGGED=None if ragged else "0"):
        data, sizes = st.encode_ragged(np.concatenate([streams[s][k] for k, s in items]),
                                       [streams[s][k].shape[0] for k, s in items], [s for _, s in items])
    grew = st.device_batches() - before
    split_frames(got, [s for _, s in items], data, sizes)
    return [bytes(g) for g in got], grew


def single_stream(level, ch, bits, blocks):
    """What the single-stream path writes for one stream fed block for block: frames, STREAMINFO bytes."""
    n = sum(b.shape[0] for b in blocks)
    with env(FLAKE_AMD_BATCH=4):
        he = V.HostEncoder(level=level, channels=ch, bits_per_sample=bits, samples=n, block_size=BS)
    with he:
        frames = b""
        for b in blocks:
            data, _ = he.encode_frames(b, b.shape[0], 0)
            frames += data.tobytes()
        si = he.streaminfo()
        buf = (C.c_ubyte * 34)()
        he.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return frames, bytes(buf)


CASES = [
    # level, channels, bits, md5 flags, verify
    (10, 2, 16, 0, True),
    (12, 2, 24, V.SET_MD5_HOST, False),
    (9, 1, 16, V.SET_MD5_OFF, True),
]


@pytest.mark.parametrize("level,ch,bits,flags,verify", CASES)
def test_closing_streams_in_one_ragged_call(level, ch, bits, flags, verify, oracle, decoder):
    streams = make_streams(level, ch, bits, oracle)
    with open_set(level, ch, bits, flags) as st:
        st.set_verify(verify)
        got, grew = close_streams(st, streams, ragged=True)
        assert st.last_verify_failure() is None
        infos = [st.streaminfo_bytes(s) for s in range(S)]
    assert grew == 1                                             # 17 tails of 17 lengths: one device batch
    with open_set(level, ch, bits, flags) as st:
        st.set_verify(verify)
        ref, ref_grew = close_streams(st, streams, ragged=False)
        ref_infos = [st.streaminfo_bytes(s) for s in range(S)]
    assert ref_grew == S
    assert got == ref and infos == ref_infos
    for s in range(S):
        whole = np.concatenate(streams[s])
        frames, si = single_stream(level, ch, bits, streams[s])
        assert got[s] == frames, (s, len(got[s]), len(frames))
        assert infos[s] == si or flags == V.SET_MD5_OFF, s
        assert infos[s][:18] == si[:18], s
        md5 = bytes(16) if flags == V.SET_MD5_OFF else hashlib.md5(packed_bytes(whole, bits)).digest()
        assert infos[s][18:] == md5, s
        if level == 10:
            pcm, _ = decoder.decode(np.frombuffer(got[s], np.uint8), ch, bits, whole.shape[0])
            assert (pcm == whole).all(), s


def test_device_batches_counts_the_chunks():
    level, ch, bits = 10, 2, 16
    streams = make_streams(level, ch, bits)
    res = {}
    for name, batch, ragged in (("batch 4", 4, True), ("default batch", None, True), ("per length", None, False)):
        with open_set(level, ch, bits, batch=batch) as st:
            assert st.device_batches() == 0
            got, grew = close_streams(st, streams, ragged=ragged)
            res[name] = (got, grew, [st.streaminfo_bytes(s) for s in range(S)])
    assert res["batch 4"][1] == 5                                # ceil(17 / 4)
    assert res["default batch"][1] == 1
    assert res["per length"][1] == S                             # 17 distinct lengths
    assert res["batch 4"][0] == res["default batch"][0] == res["per length"][0]
    assert res["batch 4"][2] == res["default batch"][2] == res["per length"][2]


def test_full_and_short_blocks_in_one_call():
    level, ch, bits = 10, 2, 16
    streams = make_streams(level, ch, bits)
    out = {}
    for ragged in (True, False):
        with open_set(level, ch, bits) as st:
            st.set_verify(ragged)
            got, grew = close_streams(st, streams, ragged=ragged, mixed=True)
            out[ragged] = (got, [st.streaminfo_bytes(s) for s in range(S)])
            # the full blocks keep their path (one batch), the short ones share one or take one per length
            assert grew == 1 + (1 if ragged else S)
    assert out[True] == out[False]
    frames, si = single_stream(level, ch, bits, streams[3])
    assert out[True][0][3] == frames and out[True][1][3] == si


def test_a_short_block_ends_nothing():
    level, ch, bits = 9, 2, 16
    streams = make_streams(level, ch, bits)
    r = np.random.RandomState(5)
    more = {s: I.burst_block(r, BS, ch, bits, 1) for s in (0, 5, 16)}
    with open_set(level, ch, bits) as st:
        st.set_verify(True)
        got, _ = close_streams(st, streams, ragged=True)
        data, sizes = st.encode(np.concatenate([more[s] for s in more]), BS, list(more))
        extra = [bytearray() for _ in range(S)]
        split_frames(extra, list(more), data, sizes)
        infos = {s: st.streaminfo_bytes(s) for s in more}
    for s in more:
        frames, si = single_stream(level, ch, bits, streams[s] + [more[s]])
        assert got[s] + bytes(extra[s]) == frames, s             # numbered from the stream's sample count
        assert infos[s] == si, s


def test_argument_errors_change_nothing():
    level, ch, bits = 10, 2, 16
    streams = make_streams(level, ch, bits)
    tail = lambda s: streams[s][-1]
    with open_set(level, ch, bits) as st:
        close_streams(st, [blocks[-1:] for blocks in streams[:3]], ragged=True)      # streams 0 .. 2 hold their tails
        state = lambda: ([st.streaminfo_bytes(s) for s in range(S)], st.device_batches())
        before = state()
        a, b = tail(2), tail(4)
        bad = [
            (np.concatenate([a, b]), [a.shape[0], b.shape[0]], [3, 3], np.int32),       # a second short block of one stream
            (np.concatenate([a, b]), [0, b.shape[0]], [3, 4], np.int32),                # a size of 0
            (np.concatenate([a, b]), [a.shape[0], b.shape[0]], [3, S], np.int32),       # a stream outside the set
            (np.concatenate([a, b]), [a.shape[0], b.shape[0]], [3, 4], np.int16),       # int16 samples
        ]
        for pcm, sizes, owners, dtype in bad:
            with pytest.raises(V.FlakeHipError):
                st.encode_ragged(pcm, sizes, owners, dtype=dtype)
            assert state() == before
        # the set is still good: the same two blocks, rightly described
        data, sizes = st.encode_ragged(np.concatenate([a, b]), [a.shape[0], b.shape[0]], [3, 4])
        assert len(data) == int(sizes.sum()) and st.device_batches() == before[1] + 1
