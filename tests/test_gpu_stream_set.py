"""The stream set of the host layer (flake_amd_set_*): many independent streams per batch, MD5s on the device.

The yardstick is the existing single-stream path, which the rest of the suite holds to the oracle: for each stream
of a set, the concatenation of its frames and its 34 STREAMINFO bytes must equal what a fresh HostEncoder writes for
that stream's samples alone (encode_frames, with the tail).  The MD5 in it must also be hashlib's over the packed
samples, and one case's streams are decoded back to the input by the spec decoder."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import flake_amd
from cases import _rng

pytestmark = pytest.mark.gpu

V = flake_amd


def packed_bytes(pcm, bits):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(pcm.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def make_streams(r, nstreams, bs, ch, bits, max_blocks):
    """Streams of unequal lengths: 0..max_blocks whole blocks plus a tail; tails come from a few shared lengths
    (so that some group) and some lengths of their own; stream 1 is empty where there is one."""
    shared = (0, 100, bs - 1, 333)
    out = []
    for s in range(nstreams):
        nblk = int(r.randint(0, max_blocks + 1))
        tail = int(shared[r.randint(0, len(shared))]) if r.randint(0, 3) else int(r.randint(1, bs))
        if s == 0:
            nblk, tail = max_blocks, 17
        if s == 1:
            nblk, tail = 0, 0
        if s in (2, 3):
            tail = 100                                          # a group of at least two
        n = nblk * bs + tail
        pcm = V.synth_pcm(nblk + 1, bs, ch, bits, first_frame=31 * s).reshape(-1, ch)[:n]
        out.append(np.ascontiguousarray(pcm))
    return out


def single_stream(level, ch, bits, pcm, bs, dtype):
    """What the single-stream path writes for one stream: frames, STREAMINFO bytes."""
    n = pcm.shape[0]
    with V.HostEncoder(level=level, channels=ch, bits_per_sample=bits, samples=n) as he:
        frames = b""
        if n:
            data, _ = (he.encode_frames_s16 if dtype == np.int16 else he.encode_frames)(pcm, bs, n % bs)
            frames = data.tobytes()
        si = he.streaminfo()
        buf = (C.c_ubyte * 34)()
        he.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return frames, bytes(buf)


def run_set(st, streams, bs, dtype, r, ncalls=3):
    """All streams through the set: the whole blocks in `ncalls` calls (round-robin layout, then seeded random
    interleavings that keep each stream's order), then the tails, grouped by length.  Returns per-stream bytes."""
    got = [bytearray() for _ in streams]
    todo = [(k, s) for s, p in enumerate(streams) for k in range(p.shape[0] // bs)]
    todo.sort()
    cuts = sorted(set([0, len(todo)] + [int(x) for x in r.randint(0, len(todo) + 1, ncalls - 1)]))
    for c, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        part = todo[a:b]
        if c % 2:
            # a random interleaving of the streams' queues
            queues = {}
            for k, s in part:
                queues.setdefault(s, []).append(k)
            lanes = [s for s, q in queues.items() for _ in q]
            r.shuffle(lanes)
            part = [(queues[s].pop(0), s) for s in lanes]
        pcm = np.concatenate([streams[s][k * bs:(k + 1) * bs] for k, s in part])
        data, sizes = st.encode(pcm, bs, [s for _, s in part], dtype=dtype)
        pos = 0
        for (_, s), fs in zip(part, sizes):
            got[s] += data[pos:pos + fs].tobytes()
            pos += fs
        assert pos == len(data)
    tails = {}
    for s, p in enumerate(streams):
        if p.shape[0] % bs:
            tails.setdefault(p.shape[0] % bs, []).append(s)
    for t, members in sorted(tails.items()):
        pcm = np.concatenate([streams[s][-t:] for s in members])
        data, sizes = st.encode(pcm, t, members, dtype=dtype)
        pos = 0
        for s, fs in zip(members, sizes):
            got[s] += data[pos:pos + fs].tobytes()
            pos += fs
    return [bytes(g) for g in got], tails


CASES = [
    # nstreams, level, channels, bits, dtype, max_blocks
    (2, 5, 2, 16, np.int32, 40),
    (17, 8, 2, 16, np.int16, 40),
    (300, 2, 2, 16, np.int16, 40),
    (300, 0, 2, 16, np.int32, 8),
    (17, 0, 2, 24, np.int32, 12),
    (17, 5, 2, 24, np.int32, 9),
    (17, 5, 8, 16, np.int32, 6),
    (2, 2, 8, 16, np.int16, 5),
    (17, 2, 2, 16, np.int32, 40),
]


@pytest.mark.parametrize("nstreams,level,ch,bits,dtype,max_blocks", CASES)
def test_set_streams_equal_single_stream_files(nstreams, level, ch, bits, dtype, max_blocks, decoder):
    r = _rng(nstreams * 100 + level * 10 + ch + bits)
    with V.StreamSet(nstreams, level=level, channels=ch, bits_per_sample=bits) as st:
        bs = st.block_size
        streams = make_streams(r, nstreams, bs, ch, bits, max_blocks)
        got, tails = run_set(st, streams, bs, dtype, r)
        assert any(len(m) > 1 for m in tails.values()) or nstreams == 2      # tails grouped by length ...
        assert any(len(m) == 1 for m in tails.values())                      # ... and alone
        infos = [st.streaminfo_bytes(s) for s in range(nstreams)]
    check = range(nstreams) if nstreams <= 17 else list(range(0, nstreams, 7)) + [1, nstreams - 1]
    for s in range(nstreams):
        # every stream's MD5 against hashlib, every stream's sample count
        assert infos[s][18:] == hashlib.md5(packed_bytes(streams[s], bits)).digest(), s
        assert struct.unpack(">I", infos[s][14:18])[0] == streams[s].shape[0], s
    for s in check:
        frames, si = single_stream(level, ch, bits, streams[s], bs, dtype)
        assert got[s] == frames, (s, len(got[s]), len(frames))
        assert infos[s] == si, s
    if nstreams == 17 and level == 5 and ch == 2:
        for s in range(nstreams):
            n = streams[s].shape[0]
            if n:
                pcm, _ = decoder.decode(np.frombuffer(got[s], np.uint8), ch, bits, n)
                assert (pcm == streams[s]).all(), s


def test_md5_flags():
    """FLAKE_AMD_SET_MD5_HOST: the same STREAMINFO bytes as the device hash (a second witness); _OFF: zeros."""
    r = _rng(3)
    S, level = 9, 2
    infos = {}
    for flags in (0, V.SET_MD5_HOST, V.SET_MD5_OFF):
        with V.StreamSet(S, level=level, flags=flags) as st:
            r2 = _rng(4)
            streams = make_streams(r2, S, st.block_size, 2, 16, 7)
            got, _ = run_set(st, streams, st.block_size, np.int16, r2)
            infos[flags] = ([st.streaminfo_bytes(s) for s in range(S)], got)
    assert infos[0] == infos[V.SET_MD5_HOST]
    assert infos[0][1] == infos[V.SET_MD5_OFF][1]
    for s in range(S):
        assert infos[V.SET_MD5_OFF][0][s][18:] == bytes(16)
        assert infos[V.SET_MD5_OFF][0][s][:18] == infos[0][0][s][:18]
        assert infos[0][0][s][18:] != bytes(16)


def test_refusals_and_the_latch():
    with pytest.raises(V.FlakeHipError, match="variable block size"):
        V.StreamSet(4, level=10)
    with pytest.raises(V.FlakeHipError, match="flags"):
        V.StreamSet(4, level=5, flags=V.SET_MD5_HOST | V.SET_MD5_OFF)
    with V.StreamSet(4, level=5, bits_per_sample=24) as st:
        with pytest.raises(V.FlakeHipError, match="int16 samples need bits_per_sample <= 16"):
            st.encode(np.zeros((st.block_size, 2), np.int16), st.block_size, [0], dtype=np.int16)
    with V.StreamSet(3, level=2) as st:
        bs = st.block_size
        pcm = V.synth_pcm(8, bs, 2, 16).reshape(-1, 2)
        ref_a, _ = single_stream(2, 2, 16, pcm[:2 * bs + 500], bs, np.int32)
        a0, sz = st.encode(pcm[:2 * bs], bs, [0, 1])
        with pytest.raises(V.FlakeHipError, match="outside the set"):
            st.encode(pcm[:2 * bs], bs, [0, 3])
        with pytest.raises(V.FlakeHipError, match="outside the set"):
            st.encode(pcm[:2 * bs], bs, [-1, 0])
        a1, _ = st.encode(pcm[2 * bs:2 * bs + 500], 500, [1])          # stream 1 ends
        before = [st.streaminfo_bytes(s) for s in range(3)]
        with pytest.raises(V.FlakeHipError, match="has ended"):
            st.encode(pcm[:2 * bs], bs, [0, 1])                        # a block behind its short block
        with pytest.raises(V.FlakeHipError, match="has ended"):
            st.encode(pcm[:1000], 500, [2, 2])                         # two short blocks for one stream
        assert [st.streaminfo_bytes(s) for s in range(3)] == before    # nothing changed for any stream
        # the set is still usable for the others: stream 0 goes on as if nothing had happened
        b0, _ = st.encode(pcm[bs:2 * bs], bs, [0])
        b1, _ = st.encode(pcm[2 * bs:2 * bs + 500], 500, [0])
        assert a0[:sz[0]].tobytes() + b0.tobytes() + b1.tobytes() == ref_a
        assert st.streaminfo_bytes(0)[18:] == hashlib.md5(packed_bytes(pcm[:2 * bs + 500], 16)).digest()
        stream1 = np.concatenate([pcm[bs:2 * bs], pcm[2 * bs:2 * bs + 500]])
        assert st.streaminfo_bytes(1)[18:] == hashlib.md5(packed_bytes(stream1, 16)).digest()
        assert a1.size > 0


def write_wav(path, pcm, bps, rate=44100):
    ch = pcm.shape[1]
    nb = (bps + 7) // 8
    raw = packed_bytes(pcm, bps)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * nb, ch * nb, bps) + b"data" +
                struct.pack("<I", len(raw)) + raw)


@pytest.mark.parametrize("bps", (16, 24))
def test_cli_set_writes_the_single_input_files(tmp_path, bps):
    cli = os.path.join(V.LIB_DIR, "flake_amd_cli")
    env = {k: v for k, v in os.environ.items() if k not in ("FLAKE_AMD_HOST_ASSEMBLY", "FLAKE_AMD_HOST_VBS")}
    lengths = (4096 * 5 + 1234, 4096 * 2, 4096 * 7 + 1234)            # two share a tail length, one has none
    outdir = tmp_path / "set"
    outdir.mkdir()
    wavs = []
    for i, n in enumerate(lengths):
        pcm = V.synth_pcm(8, 4096, 2, bps, first_frame=11 * i).reshape(-1, 2)[:n]
        w = tmp_path / f"in{i}.wav"
        write_wav(w, pcm, bps)
        wavs.append(str(w))
        r = subprocess.run([cli, "-5", str(w), str(tmp_path / f"single{i}.flac")], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    r = subprocess.run([cli, "-5", "--set", str(outdir), *wavs], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for i in range(len(lengths)):
        a = (tmp_path / f"single{i}.flac").read_bytes()
        b = (outdir / f"in{i}.flac").read_bytes()
        assert a == b, (i, len(a), len(b))
