"""flake_amd_set_encode_ragged: the tails of many streams, all of different lengths, in one call.

The yardstick is the code that already exists.  For every stream of a set closed through the ragged entry, the
concatenation of its frames and its 34 STREAMINFO bytes must equal (a) what a fresh single-stream HostEncoder writes
for that stream's samples alone and (b) what a second set writes that ends its streams with one flake_amd_set_encode
call per tail length.  The MD5 must be hashlib's.  Block sizes are small (params.block_size 256 and 1152) so that a
case is a few dozen short frames; the tail lengths of every call include the lengths at which the generic code
branches: 1..5 (warm-up longer than the block, verbatim below 5), 31/32/33 (the stereo estimate's gate),
max_prediction_order and one more (LPC against fixed), an odd length, one that is 2 mod 4 (int16 blocks then start at
2-byte boundaries for odd channel counts), block_size - 1, and lengths on both sides of 256 (the header's 8- and
16-bit size fields) where the block size allows.

The cases are a covering selection of channels {1, 2, 3} x {16 bits as int16, 16 bits as int32, 24 bits} x levels
{0, 2, 5, 8} x MD5 {device, host, off} x verify {off, on}: every value of every dimension occurs, each channel
count with each sample format, each level with verification on and off."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import flake_amd
from cases import _rng

pytestmark = pytest.mark.gpu

V = flake_amd


def packed_bytes(pcm, bits):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(pcm.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def tail_lengths(bs, max_order):
    want = [1, 2, 3, 4, 5, 31, 32, 33, max_order, max_order + 1, 77, 102, bs - 1, 200, 255]
    if bs > 300:
        want += [256, 257, 300, 1000]
    out = []
    for t in want:
        if 1 <= t < bs and t not in out:
            out.append(t)
    return out


def make_streams(bs, ch, bits, tails):
    """Stream s: s % 3 whole blocks, then tails[s] samples."""
    out = []
    for s, t in enumerate(tails):
        nblk = s % 3
        n = nblk * bs + t
        pcm = V.synth_pcm(nblk + 1, bs, ch, bits, first_frame=17 * s + 3).reshape(-1, ch)[:n]
        out.append(np.ascontiguousarray(pcm))
    return out


def single_stream(level, ch, bits, pcm, bs, dtype):
    """What the single-stream path writes for one stream: frames, STREAMINFO bytes (a helper of this file's own,
    after test_gpu_stream_set.single_stream, with the block size overridden)."""
    n = pcm.shape[0]
    with V.HostEncoder(level=level, channels=ch, bits_per_sample=bits, samples=n, block_size=bs) as he:
        data, _ = (he.encode_frames_s16 if dtype == np.int16 else he.encode_frames)(pcm, bs, n % bs)
        si = he.streaminfo()
        buf = (C.c_ubyte * 34)()
        he.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return data.tobytes(), bytes(buf)


def split_frames(got, members, data, sizes):
    pos = 0
    for s, fs in zip(members, sizes):
        got[s] += data[pos:pos + fs].tobytes()
        pos += int(fs)
    assert pos == len(data)


def whole_blocks(st, streams, bs, dtype, got):
    part = [(k, s) for s, p in enumerate(streams) for k in range(p.shape[0] // bs)]
    part.sort()
    if part:
        pcm = np.concatenate([streams[s][k * bs:(k + 1) * bs] for k, s in part])
        data, sizes = st.encode(pcm, bs, [s for _, s in part], dtype=dtype)
        split_frames(got, [s for _, s in part], data, sizes)


def close_ragged(st, streams, bs, dtype, mixed=False):
    """The set's streams through the ragged entry: the tails in ONE call -- with `mixed`, the whole blocks in that
    call too, every stream's blocks in stream order and interleaved with the others'."""
    got = [bytearray() for _ in streams]
    if mixed:
        items = [(k, s) for s, p in enumerate(streams) for k in range((p.shape[0] + bs - 1) // bs)]
        items.sort()                                             # block k of every stream, then block k + 1
    else:
        whole_blocks(st, streams, bs, dtype, got)
        items = [(p.shape[0] // bs, s) for s, p in enumerate(streams)]
    pcm = np.concatenate([streams[s][k * bs:(k + 1) * bs] for k, s in items])
    sizes_in = [min(bs, streams[s].shape[0] - k * bs) for k, s in items]
    data, sizes = st.encode_ragged(pcm, sizes_in, [s for _, s in items], dtype=dtype)
    split_frames(got, [s for _, s in items], data, sizes)
    return [bytes(g) for g in got]


def close_per_length(st, streams, bs, dtype):
    got = [bytearray() for _ in streams]
    whole_blocks(st, streams, bs, dtype, got)
    for s, p in enumerate(streams):
        t = p.shape[0] % bs
        data, sizes = st.encode(p[-t:], t, [s], dtype=dtype)
        split_frames(got, [s], data, sizes)
    return [bytes(g) for g in got]


MD5_DEV = 0
CASES = [
    # bs, level, channels, bits, dtype, md5 flags, verify
    (256, 5, 2, 16, np.int16, MD5_DEV, False),
    (256, 5, 2, 16, np.int32, MD5_DEV, True),
    (1152, 8, 2, 16, np.int16, MD5_DEV, True),
    (1152, 8, 2, 24, np.int32, V.SET_MD5_HOST, False),
    (256, 0, 1, 16, np.int16, V.SET_MD5_OFF, True),
    (256, 0, 2, 24, np.int32, MD5_DEV, False),
    (1152, 2, 1, 24, np.int32, MD5_DEV, True),
    (256, 2, 3, 16, np.int16, MD5_DEV, False),
    (1152, 5, 3, 16, np.int32, V.SET_MD5_HOST, True),
    (256, 5, 3, 24, np.int32, V.SET_MD5_OFF, False),
    (1152, 5, 1, 16, np.int32, MD5_DEV, False),
    (1152, 2, 2, 16, np.int16, V.SET_MD5_HOST, True),
    (256, 8, 1, 16, np.int16, MD5_DEV, False),
    (1152, 0, 3, 16, np.int16, MD5_DEV, True),
]


@pytest.mark.parametrize("bs,level,ch,bits,dtype,flags,verify", CASES)
def test_ragged_tails_equal_single_streams_and_per_length_calls(bs, level, ch, bits, dtype, flags, verify, decoder):
    with V.StreamSet(1, level=level, channels=ch, bits_per_sample=bits, block_size=bs) as probe:
        max_order = probe.ctx.params.max_prediction_order
    tails = tail_lengths(bs, max_order)
    for need in (1, 2, 3, 4, 5, 31, 32, 33, max_order, max_order + 1, bs - 1):
        assert need in tails or need < 1
    assert any(t % 2 for t in tails) and any(t % 4 == 2 for t in tails)
    streams = make_streams(bs, ch, bits, tails)
    S = len(streams)
    results = []
    for close in (close_ragged, close_per_length):
        with V.StreamSet(S, level=level, channels=ch, bits_per_sample=bits, flags=flags, block_size=bs) as st:
            assert st.block_size == bs
            st.set_verify(verify)
            got = close(st, streams, bs, dtype)
            results.append((got, [st.streaminfo_bytes(s) for s in range(S)]))
    (got, infos), (got2, infos2) = results
    assert got == got2
    assert infos == infos2
    for s in range(S):
        frames, si = single_stream(level, ch, bits, streams[s], bs, dtype)
        assert got[s] == frames, (s, tails[s], len(got[s]), len(frames))
        if flags == MD5_DEV:
            assert infos[s] == si, (s, tails[s])
            assert infos[s][18:] == hashlib.md5(packed_bytes(streams[s], bits)).digest(), s
        elif flags == V.SET_MD5_HOST:
            assert infos[s] == si, (s, tails[s])
        else:
            assert infos[s][:18] == si[:18] and infos[s][18:] == bytes(16), s
        assert struct.unpack(">I", infos[s][14:18])[0] == streams[s].shape[0], s
    if verify:
        for s in range(S):
            pcm, _ = decoder.decode(np.frombuffer(got[s], np.uint8), ch, bits, streams[s].shape[0])
            assert (pcm == streams[s]).all(), (s, tails[s])


@pytest.mark.parametrize("dtype,verify", [(np.int16, False), (np.int32, True)])
def test_full_and_short_blocks_share_one_call(dtype, verify):
    bs, level, ch, bits = 256, 5, 2, 16
    tails = tail_lengths(bs, 8)
    streams = make_streams(bs, ch, bits, tails)
    assert any(p.shape[0] // bs == 2 for p in streams)           # streams that get whole blocks AND a tail in the call
    with V.StreamSet(len(streams), level=level, block_size=bs) as st:
        st.set_verify(verify)
        got = close_ragged(st, streams, bs, dtype, mixed=True)
        infos = [st.streaminfo_bytes(s) for s in range(len(streams))]
    for s, p in enumerate(streams):
        frames, si = single_stream(level, ch, bits, p, bs, dtype)
        assert got[s] == frames, (s, tails[s])
        assert infos[s] == si, (s, tails[s])


def test_a_single_stream_with_a_single_tail():
    bs = 256
    pcm = V.synth_pcm(1, bs, 2, 16, first_frame=5).reshape(-1, 2)[:77]
    with V.StreamSet(1, level=5, block_size=bs) as st:
        data, sizes = st.encode_ragged(pcm, [77], [0])
        info = st.streaminfo_bytes(0)
    frames, si = single_stream(5, 2, 16, pcm, bs, np.int32)
    assert data.tobytes() == frames and list(sizes) == [len(frames)]
    assert info == si


def test_the_comparison_leg_writes_the_same_bytes(monkeypatch):
    """FLAKE_AMD_SET_RAGGED=0: one uniform call per distinct length, the same files."""
    bs, level, ch, bits = 256, 5, 2, 16
    tails = tail_lengths(bs, 8) + [77, 5]                        # (lengths that two streams share)
    streams = make_streams(bs, ch, bits, tails)
    out = {}
    for leg in ("1", "0"):
        monkeypatch.setenv("FLAKE_AMD_SET_RAGGED", leg)
        with V.StreamSet(len(streams), level=level, block_size=bs) as st:
            out[leg] = (close_ragged(st, streams, bs, np.int16, mixed=True),
                        [st.streaminfo_bytes(s) for s in range(len(streams))])
    assert out["0"] == out["1"]
    frames, si = single_stream(level, ch, bits, streams[3], bs, np.int16)
    assert out["0"][0][3] == frames and out["0"][1][3] == si


def test_refusals_change_no_stream():
    bs = 256
    pcm = V.synth_pcm(4, bs, 2, 16).reshape(-1, 2)
    with V.StreamSet(3, level=2, block_size=bs) as st:
        st.encode(pcm[:2 * bs], bs, [0, 1])
        st.encode_ragged(pcm[:100], [100], [1])                                     # stream 1 ends
        before = [st.streaminfo_bytes(s) for s in range(3)]
        with pytest.raises(V.FlakeHipError, match="has ended"):
            st.encode_ragged(pcm[:150], [100, 50], [2, 2])                          # two short blocks for one stream
        with pytest.raises(V.FlakeHipError, match="has ended"):
            st.encode_ragged(pcm[:100 + bs], [100, bs], [0, 0])                     # a block behind a tail
        with pytest.raises(V.FlakeHipError, match="has ended"):
            st.encode_ragged(pcm[:bs + 7], [bs, 7], [0, 1])                         # ... behind an earlier call's tail
        with pytest.raises(V.FlakeHipError, match="outside the set"):
            st.encode_ragged(pcm[:150], [100, 50], [0, 3])
        with pytest.raises(V.FlakeHipError, match="outside the set"):
            st.encode_ragged(pcm[:150], [100, 50], [-1, 0])
        with pytest.raises(V.FlakeHipError, match="out of range"):
            st.encode_ragged(pcm[:100], [100, 0], [0, 2])
        with pytest.raises(V.FlakeHipError, match="out of range"):
            st.encode_ragged(pcm[:100 + bs + 1], [100, bs + 1], [0, 2])
        assert [st.streaminfo_bytes(s) for s in range(3)] == before
        # the set goes on as if nothing had happened
        a, _ = st.encode_ragged(pcm[2 * bs:3 * bs + 33], [bs, 33], [0, 0])
        ref, si = single_stream(2, 2, 16, np.concatenate([pcm[:bs], pcm[2 * bs:3 * bs + 33]]), bs, np.int32)
        first, _ = single_stream(2, 2, 16, pcm[:bs], bs, np.int32)
        assert first + a.tobytes() == ref
        assert st.streaminfo_bytes(0) == si
