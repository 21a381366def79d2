"""Stream sets with variable block size (FLAKE_AMD_SET_VBS, levels 9-12): many streams per batch, a block may become
several frames, frames numbered by their stream's sample count.

The yardstick is the single-stream path, which the rest of the suite holds to the oracle: each stream's concatenated
frames and its 34 STREAMINFO bytes must equal what a fresh HostEncoder at the same level writes when it is fed that
stream alone, block for block; each MD5 must be hashlib's.  The signal is bursts against near-silence per eighth of
a block, so that split_frame_v1 (the oracle's, on the CPU) splits a good part of the blocks and leaves others whole:
a case asserts that before it trusts itself.

Run as a program (python test_gpu_set_vbs.py CASE) it runs one case of the byte test: the child of the
FLAKE_AMD_BATCH=64 test."""
import contextlib
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":          # (pytest's conftest does this for the suite)
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import flake_amd
from cases import _rng
from test_set_verify_map_cpu import block_of_frame

pytestmark = pytest.mark.gpu

V = flake_amd


@pytest.fixture(scope="module", autouse=True)
def torch():
    # (autouse: torch brings a HIP runtime of its own and finds no device when it starts after libflakehip.so has
    # initialised the other one in this process -- it comes first, as in the modules whose first test asks for it)
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def packed_bytes(pcm, bits):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(pcm.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def burst_block(r, n, ch, bits, kind):
    """One block of n samples: every eighth is a noise burst or near-silence.  kind 0: all eighths loud alike (the
    splitter leaves such a block whole), else a pattern with at least one change (it cuts there)."""
    loud, quiet = 1 << (bits - 3), 3
    e = max(n // 8, 1)
    pat = np.ones(8, np.int64)
    if kind:
        while pat.min() == pat.max():
            pat = r.randint(0, 2, 8)
    amp = np.where(np.repeat(pat, e)[:n] > 0, loud, quiet) if n >= 8 else np.full(n, loud)
    amp = np.concatenate([amp, np.full(n - len(amp), amp[-1] if len(amp) else loud)])
    base = (r.uniform(-1.0, 1.0, n) * amp).astype(np.int64)
    out = np.empty((n, ch), np.int32)
    for c in range(ch):
        # channels alike but not equal: stereo decorrelation has something to decide
        out[:, c] = base + (r.uniform(-1.0, 1.0, n) * np.maximum(amp // 16, 1)).astype(np.int64)
    lim = (1 << (bits - 1)) - 1
    return np.clip(out, -lim - 1, lim)


def make_stream(r, lengths, ch, bits, whole_every=3):
    """A stream as the list of its blocks (each [n][ch] int32), one per entry of lengths."""
    return [burst_block(r, n, ch, bits, 0 if r.randint(0, whole_every) == 0 else 1) for n in lengths]


def stream_lengths(r, nstreams, bs, max_blocks, tails):
    """Unequal streams: 0..max_blocks whole blocks plus a tail of one of four kinds -- a multiple of 8 that split_frame_v1
    takes (>= 128), a multiple of 8 below 128, an odd length, none.  Stream 1 is empty (of more than two); stream 2 has two short blocks
    (in separate calls: no latch with allow_vbs) and stream 3 a whole block behind its short one."""
    out = []
    for s in range(nstreams):
        ln = [bs] * int(r.randint(0, max_blocks + 1))
        t = tails[int(r.randint(0, len(tails)))]
        if s == 0:
            ln, t = [bs] * max_blocks, tails[2]
        if s == 1:
            ln, t = [], 0
        if t:
            ln.append(t)
        if s == 1 and nstreams == 2:
            ln = [bs, bs, bs, tails[0], tails[2]]          # (two streams: none is empty, or nothing would interleave)
        if s == 2:
            ln = [bs, tails[0], tails[2]]
        if s == 3:
            ln = [bs, tails[1], bs]
        out.append(ln)
    return out


@contextlib.contextmanager
def small_batches(blocks):
    """The reference encoders see a few blocks each: size their workspaces for that (the bytes do not depend on it)."""
    old = os.environ.get("FLAKE_AMD_BATCH")
    os.environ["FLAKE_AMD_BATCH"] = str(max(int(blocks), 1))
    try:
        yield
    finally:
        if old is None:
            del os.environ["FLAKE_AMD_BATCH"]
        else:
            os.environ["FLAKE_AMD_BATCH"] = old


def single_stream(level, ch, bits, blocks):
    """What the single-stream path writes for one stream fed block for block: frames, STREAMINFO bytes."""
    n = sum(b.shape[0] for b in blocks)
    with small_batches(len(blocks)):
        he = V.HostEncoder(level=level, channels=ch, bits_per_sample=bits, samples=n)
    with he:
        frames = b""
        i = 0
        while i < len(blocks):
            j = i
            while j < len(blocks) and blocks[j].shape[0] == blocks[i].shape[0]:
                j += 1
            data, _ = he.encode_frames(np.concatenate(blocks[i:j]), blocks[i].shape[0], 0)
            frames += data.tobytes()
            i = j
        si = he.streaminfo()
        buf = (C.c_ubyte * 34)()
        he.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return frames, bytes(buf)


def plan_calls(streams, bs, r):
    """The calls that take all streams through a set: each a (block length or None for a ragged call, [(stream, block
    index)]).  A call takes blocks of one length from the heads of the streams' queues -- of the whole blocks a random
    share of each stream's run, so that they spread over several calls -- in a seeded random interleaving that keeps
    each stream's order.  The first round in which every head is short, of several lengths, is one ragged call."""
    head = [0] * len(streams)
    calls = []
    ragged_done = False
    while True:
        heads = {}
        for s, blocks in enumerate(streams):
            if head[s] < len(blocks):
                heads.setdefault(blocks[head[s]].shape[0], []).append(s)
        if not heads:
            return calls
        if bs not in heads and len(heads) > 1 and not ragged_done:
            ragged_done = True
            part = [(s, head[s]) for m in heads.values() for s in m]
            r.shuffle(part)
            n = None
        else:
            n = bs if bs in heads else sorted(heads)[0]
            lanes = []
            for s in heads[n]:
                run = 0
                while head[s] + run < len(streams[s]) and streams[s][head[s] + run].shape[0] == n:
                    run += 1
                lanes += [s] * (int(r.randint(1, run + 1)) if n == bs else 1)
            r.shuffle(lanes)
            taken = {}
            part = []
            for s in lanes:
                part.append((s, head[s] + taken.get(s, 0)))
                taken[s] = taken.get(s, 0) + 1
        for s, k in part:
            head[s] = k + 1
        calls.append((n, part))


def run_set(st, streams, calls):
    """The planned calls through the set; returns the per-stream bytes."""
    got = [bytearray() for _ in streams]
    for n, part in calls:
        pcm = np.concatenate([streams[s][k] for s, k in part])
        if n is None:
            data, sizes = st.encode_ragged(pcm, [streams[s][k].shape[0] for s, k in part], [s for s, _ in part])
        else:
            data, sizes = st.encode(pcm, n, [s for s, _ in part])
        pos = 0
        for (s, k), fs in zip(part, sizes):
            got[s] += data[pos:pos + fs].tobytes()
            pos += int(fs)
        assert pos == len(data)
    return [bytes(g) for g in got]


def case_streams(nstreams, level, ch, bits, max_blocks, bs):
    r = _rng(7000 + nstreams * 100 + level * 10 + ch + bits)
    lengths = stream_lengths(r, nstreams, bs, max_blocks, tails_for(level))
    streams = [make_stream(r, ln, ch, bits) for ln in lengths]
    return streams, plan_calls(streams, bs, r)


def exercises_the_table(oracle, streams, calls, ch, bs):
    """Of the whole blocks at least a quarter are split and one is not, and some split block is not the first stream's
    of its call -- by split_frame_v1 itself, on the CPU; the whole blocks take at least two calls."""
    nf = {(s, k): oracle.vbs_split(b, ch, bs)[0] for s, blocks in enumerate(streams)
          for k, b in enumerate(blocks) if b.shape[0] == bs}
    split = [key for key, f in nf.items() if f > 1]
    assert len(split) * 4 >= len(nf) and len(split) < len(nf), (len(split), len(nf))
    assert any(nf.get(key, 1) > 1 and key[0] != part[0][0] for n, part in calls if n == bs for key in part)
    assert sum(1 for n, _ in calls if n == bs) >= 2 and any(n is None for n, _ in calls)


CASES = [
    # nstreams, level, channels, bits, max_blocks
    (2, 10, 2, 16, 6),
    (17, 9, 2, 16, 4),
    (17, 12, 2, 24, 2),
    (9, 11, 8, 16, 2),
    (300, 10, 1, 16, 3),
]


def tails_for(level):
    # levels 11 / 12 search up to order 32: every piece holds at least 64 samples
    return (1024, 104, 333, 0) if level >= 11 else (1000, 104, 333, 0)


def byte_case(nstreams, level, ch, bits, max_blocks, oracle, decoder=None):
    with V.StreamSet(nstreams, level=level, channels=ch, bits_per_sample=bits, flags=V.SET_VBS) as st:
        bs = st.block_size
        st.set_verify(level in (9, 11))          # (the bytes are the single stream's with verification on or off)
        streams, calls = case_streams(nstreams, level, ch, bits, max_blocks, bs)
        exercises_the_table(oracle, streams, calls, ch, bs)
        got = run_set(st, streams, calls)
        infos = [st.streaminfo_bytes(s) for s in range(nstreams)]
    for s in range(nstreams):
        whole = np.concatenate(streams[s]) if streams[s] else np.zeros((0, ch), np.int32)
        assert infos[s][18:] == hashlib.md5(packed_bytes(whole, bits)).digest(), s
        assert struct.unpack(">I", infos[s][14:18])[0] == whole.shape[0], s
        frames, si = single_stream(level, ch, bits, streams[s])
        assert got[s] == frames, (s, len(got[s]), len(frames))
        assert infos[s] == si, s
        if decoder is not None and whole.shape[0]:
            pcm, _ = decoder.decode(np.frombuffer(got[s], np.uint8), ch, bits, whole.shape[0])
            assert (pcm == whole).all(), s


@pytest.mark.parametrize("nstreams,level,ch,bits,max_blocks", CASES)
def test_set_streams_equal_single_stream_files(nstreams, level, ch, bits, max_blocks, oracle, decoder):
    byte_case(nstreams, level, ch, bits, max_blocks, oracle, decoder if (nstreams, level) == (17, 9) else None)


def test_md5_modes_agree():
    """The host hash and no hash: the same frames, the same STREAMINFO up to the signature."""
    res = {}
    for flags in (0, V.SET_MD5_HOST, V.SET_MD5_OFF):
        r = _rng(11)
        with V.StreamSet(5, level=9, flags=flags | V.SET_VBS) as st:
            bs = st.block_size
            streams = [make_stream(r, ln, 2, 16) for ln in stream_lengths(r, 5, bs, 2, tails_for(9))]
            got = run_set(st, streams, plan_calls(streams, bs, r))
            res[flags] = ([st.streaminfo_bytes(s) for s in range(5)], got)
    assert res[0] == res[V.SET_MD5_HOST]
    assert res[0][1] == res[V.SET_MD5_OFF][1]
    for s in range(5):
        assert res[V.SET_MD5_OFF][0][s][18:] == bytes(16)
        assert res[V.SET_MD5_OFF][0][s][:18] == res[0][0][s][:18]


# ---- chunk edges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [None, "2048"])
def test_more_than_1024_blocks_and_frames_in_one_call(batch, oracle, monkeypatch):
    """1100 blocks of 128 samples in one call over 37 streams, verification on: more blocks than the plan kernel's
    chunk of 1024 (with FLAKE_AMD_BATCH=2048 they reach it in one launch; by default the set's own loop cuts the call
    at 1024) and more frames than K5's chunk."""
    if batch:
        monkeypatch.setenv("FLAKE_AMD_BATCH", batch)
    S, NB, n, level = 37, 1100, 128, 10
    r = _rng(4242)
    owner = r.randint(0, S, NB)                     # (a stream's blocks are in its order wherever they lie)
    blocks = [burst_block(r, n, 2, 16, 0 if b % 3 == 0 else 1) for b in range(NB)]
    assert sum(oracle.vbs_split(b, 2, n)[0] for b in blocks) > 1024
    with V.StreamSet(S, level=level, flags=V.SET_VBS) as st:
        assert n < st.block_size
        st.set_verify(True)
        data, sizes = st.encode(np.concatenate(blocks), n, owner)
        infos = [st.streaminfo_bytes(s) for s in range(S)]
    monkeypatch.delenv("FLAKE_AMD_BATCH", raising=False)
    got = [bytearray() for _ in range(S)]
    pos = 0
    for b in range(NB):
        got[owner[b]] += data[pos:pos + sizes[b]].tobytes()
        pos += int(sizes[b])
    assert pos == len(data)
    for s in range(S):
        mine = [blocks[b] for b in range(NB) if owner[b] == s]
        frames, si = single_stream(level, 2, 16, mine)
        assert bytes(got[s]) == frames, s
        assert infos[s] == si, s


def test_chunks_of_64_commit_across_chunks():
    """One case of the byte test with FLAKE_AMD_BATCH=64, in a child process: the set's own chunk loop."""
    env = dict(os.environ, FLAKE_AMD_BATCH="64")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "4"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=HERE)
    assert r.returncode == 0 and "case ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- the verifier's block-table mode ------------------------------------------------------------------------------

def twelve_blocks(oracle):
    """A set's output for 12 blocks of 4 streams in one call, with every frame's size (the oracle's, which the output
    is held to here), the blocks' first-sample numbers and their streams."""
    level, ch, bits, S = 10, 2, 16, 4
    p = V.level_params(level)
    bs = p.block_size
    r = _rng(99)
    owner = [0, 1, 2, 3, 1, 0, 3, 2, 2, 1, 0, 3]
    blocks = [burst_block(r, bs, ch, bits, 0 if b in (2, 7) else 1) for b in range(12)]
    pcm = np.concatenate(blocks)
    with V.StreamSet(S, level=level, flags=V.SET_VBS) as st:
        data, sizes = st.encode(pcm, bs, owner)
    with V.StreamSet(S, level=level, flags=V.SET_VBS) as st:
        st.set_verify(True)
        data2, sizes2 = st.encode(pcm, bs, owner)
        assert st.last_verify_failure() is None
    assert np.array_equal(data, data2) and np.array_equal(sizes, sizes2)      # the same bytes with verification on
    seen = [0] * S
    first, fbytes, nfr = [], [], []
    exp = b""
    for b in range(12):
        first.append(seen[owner[b]] * bs)
        seen[owner[b]] += 1
        nf, psz = oracle.vbs_split(blocks[b], ch, bs)
        if nf <= 1:
            psz = [bs]
        at = 0
        for q in psz:
            rc, out, _, _, _ = oracle.encode_frame(p, first[b] + at, blocks[b][at:at + q], int(q))
            assert rc > 0
            fbytes.append(rc)
            exp += out.tobytes()
            at += int(q)
        nfr.append(len(psz))
    assert data.tobytes() == exp
    return dict(p=p, bs=bs, pcm=pcm, data=data, fbytes=np.array(fbytes, np.int32), first=np.array(first, np.uint32),
                nfr=nfr, owner=owner, start=np.concatenate([[0], np.cumsum(nfr)]))


@pytest.fixture(scope="module")
def twelve(oracle):
    return twelve_blocks(oracle)


def first_failure(recs):
    bad = np.nonzero(recs["status"] != 0)[0]
    return int(bad[0]) if len(bad) else -1


def test_block_table_verifier(twelve, torch):
    t = twelve
    nf = len(t["fbytes"])
    with V.Encoder(t["p"], max_frames=96) as enc:
        ok, recs, summ, err = enc.verify_frames_blocks(t["data"], t["fbytes"], t["pcm"], t["first"], t["bs"])
        assert ok, err
        assert summ[0] == nf and summ[1] == 0 and summ[2] == -1 and np.all(recs["status"] == 0)

        def both(stream, fb, first, nblocks=None):
            """The host entry's records; the _dev twin must give the same."""
            ok, recs, summ, err = enc.verify_frames_blocks(stream, fb, t["pcm"], first, t["bs"], nblocks)
            dev = torch.device("cuda")
            ds = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
            dfb = torch.from_numpy(np.ascontiguousarray(fb, np.int32)).to(dev)
            dp = torch.from_numpy(np.ascontiguousarray(t["pcm"], np.int32).reshape(-1)).to(dev)
            dbf = torch.from_numpy(np.ascontiguousarray(first, np.uint32).view(np.int32)).to(dev)
            dsum = torch.full((4,), 99, dtype=torch.int64, device=dev)
            drec = torch.zeros((len(fb), 4), dtype=torch.int32, device=dev)
            enc.verify_frames_blocks_dev(ds, len(stream), dfb, len(fb), dp, t["pcm"].shape[0], dbf,
                                         len(first) if nblocks is None else nblocks, t["bs"], dsum, drec)
            enc.sync()
            assert np.array_equal(dsum.cpu().numpy(), summ)
            assert np.array_equal(drec.cpu().numpy().reshape(-1), recs.view(np.int32).reshape(-1))
            assert not ok and summ[2] == first_failure(recs)
            return recs, summ, err

        # block 5's table entry off by one: its first frame does not carry the number, nothing before it is flagged
        bad = t["first"].copy()
        bad[5] += 1
        recs, summ, err = both(t["data"], t["fbytes"], bad)
        f5 = int(t["start"][5])
        assert summ[2] == f5 and recs["status"][f5] == V.V_NUMBER and recs["bit"][f5] == 32
        assert f"number {int(bad[5])}" in err
        assert enc.last_verify_failure()[2] == int(bad[5])

        # two whole blocks of different streams, of equal frame counts, swapped in the stream
        pair = [(i, j) for i in range(12) for j in range(i + 1, 12)
                if t["nfr"][i] == t["nfr"][j] and t["owner"][i] != t["owner"][j] and t["first"][i] != t["first"][j]]
        assert pair
        i, j = pair[0]
        off = np.concatenate([[0], np.cumsum(t["fbytes"])])
        seg = lambda b: t["data"][off[t["start"][b]]:off[t["start"][b + 1]]]
        fseg = lambda b: t["fbytes"][t["start"][b]:t["start"][b + 1]]
        order = list(range(12))
        order[i], order[j] = j, i
        recs, summ, _ = both(np.concatenate([seg(b) for b in order]), np.concatenate([fseg(b) for b in order]), t["first"])
        fi = int(t["start"][i])
        assert summ[2] == fi and recs["status"][fi] in (V.V_NUMBER, V.V_SAMPLES)

        # one byte of a residual flipped
        f = int(t["start"][6])
        hurt = t["data"].copy()
        hurt[off[f] + (3 * int(t["fbytes"][f])) // 4] ^= 0x10
        recs, summ, _ = both(hurt, t["fbytes"], t["first"])
        assert summ[2] == f and summ[1] == 1 and recs["status"][f] in (V.V_SAMPLES, V.V_CRC16)

        # a table one block short: the last block's frames lie in no block
        recs, summ, _ = both(t["data"], t["fbytes"], t["first"], nblocks=11)
        f11 = int(t["start"][11])
        assert summ[2] == f11 and recs["status"][f11] == V.V_NUMBER and recs["bit"][f11] == 16
        assert np.all(recs["status"][:f11] == 0)


def test_set_level_failure_names_stream_and_sample(twelve):
    """What flake_amd_set_encode relays when a chunk fails: the first failing frame, mapped to its block by the prefix
    sum of block_frames (fa_block_of_frame; test_set_verify_map_cpu.py runs the C) and from there to its stream, and the first-sample number it had to carry
    (fhip_last_verify_number).  The encoder cannot be made to fail from outside without breaking it -- K4 writes what
    the table says and K5 is given the same table -- so the verdict is provoked where a table can be wrong: the entry
    the set encodes through writes the batch by one table, and the verifier is handed another."""
    t = twelve
    with V.Encoder(t["p"], max_frames=96) as enc:
        enc.set_verify(True)
        data, bb, bfr, bmx = enc.encode_blocks_vbs_packed_numbered(t["pcm"], t["bs"], t["first"])
        assert np.array_equal(data, t["data"]) and list(bfr) == t["nfr"]
        assert [int(x) for x in bmx] == [int(t["fbytes"][a:b].max()) for a, b in zip(t["start"][:-1], t["start"][1:])]
        assert enc.last_verify_failure() is None
        wrong = t["first"].copy()
        wrong[7] += 8
        data_w, _, bfr_w, _ = enc.encode_blocks_vbs_packed_numbered(t["pcm"], t["bs"], wrong)   # consistent: passes
        assert list(bfr_w) == t["nfr"] and not np.array_equal(data_w, data)
        ok, recs, summ, err = enc.verify_frames_blocks(data_w, t["fbytes"], t["pcm"], t["first"], t["bs"])
        assert not ok
        summary, rec, number = enc.last_verify_failure()
        blk = block_of_frame(bfr_w, int(summary[2]))      # flake_set.c's map, held to this expression on the CPU
        assert blk == 7 and t["owner"][blk] == 2 and rec["status"] == V.V_NUMBER and rec["bit"] == 32
        assert number == int(t["first"][7]) == t["bs"]          # stream 2's second block: its sample 4096


# ---- refusals and unchanged behaviour -----------------------------------------------------------------------------

def test_refusals():
    with pytest.raises(V.FlakeHipError, match="variable block size"):
        V.StreamSet(4, level=10)
    with pytest.raises(V.FlakeHipError, match="FLAKE_AMD_SET_VBS"):
        V.StreamSet(4, level=5, flags=V.SET_VBS)
    with V.StreamSet(4, level=10, flags=V.SET_VBS) as st:
        with pytest.raises(V.FlakeHipError, match="int16"):
            st.encode(np.zeros((st.block_size, 2), np.int16), st.block_size, [0], dtype=np.int16)
        assert st.streaminfo(0).min_block_size == 16
    with V.Encoder(V.level_params(5), max_frames=8) as enc:
        assert enc.lib.fhip_set_block_numbering(enc._h, 1) == V.E_UNSUPPORTED
        s = np.zeros(4, np.int64)
        vi = V.VerifyIn(None, 0, None, 0, None, 0, 0)
        vo = V.VerifyOut(None, s.ctypes.data)
        assert enc.lib.fhip_verify_frames_blocks(enc._h, C.byref(vi), None, 0, 4096, C.byref(vo)) == V.E_UNSUPPORTED


def test_single_stream_entries_launch_what_they_launched(torch):
    """fhip_encode_blocks_vbs_packed and _dev: the same bytes as each other and the kernel list of a batch without a
    table -- k_vbs_plan, k_vbs_block_bytes and K5's header pass under their plain names, no table instance."""
    p = V.level_params(10)
    n, nb = p.block_size, 8
    r = _rng(5)
    pcm = np.concatenate([burst_block(r, n, 2, 16, b % 2) for b in range(nb)])
    with V.Encoder(p, max_frames=8 * nb) as enc:
        enc.set_verify(True)
        cap = pcm.size * 5 + 4096
        out = np.zeros(cap, np.uint8)
        bb = np.zeros(nb, np.int32)
        wrote, mx, nxt = C.c_int64(0), C.c_int(0), C.c_uint32(0)
        rc = enc.lib.fhip_encode_blocks_vbs_packed(enc._h, pcm.ctypes.data, nb, n, 3 * n, out.ctypes.data, cap,
                                                   bb.ctypes.data, None, C.byref(wrote), C.byref(mx), C.byref(nxt))
        assert rc == 0, enc.lib.fhip_last_error(enc._h)
        packed_list = enc.last_launches()
        dev = torch.device("cuda")
        dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
        dpk = torch.zeros(cap, dtype=torch.uint8, device=dev)
        dt = torch.zeros(4, dtype=torch.int64, device=dev)
        dbb = torch.zeros(nb, dtype=torch.int32, device=dev)
        enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt, block_bytes=dbb, first_frame_number=3 * n)
        enc.sync()
        dev_list = enc.last_launches()
        assert np.array_equal(dpk.cpu().numpy()[:int(dt[1])], out[:wrote.value]) and int(dt[3]) == 0
        assert np.array_equal(dbb.cpu().numpy(), bb)
        assert packed_list == dev_list
        for name in ("k_vbs_plan", "k_vbs_block_bytes", "k_verify_frames"):
            assert packed_list.count(name) == 1, packed_list
        assert not any("<block_first>" in x or "<blocks>" in x for x in packed_list)
        # the table entry with the single stream's numbers writes the single stream's bytes, through the table instances
        first = (3 * n + n * np.arange(nb)).astype(np.uint32)
        data, bb2, _, _ = enc.encode_blocks_vbs_packed_numbered(pcm, n, first)
        assert np.array_equal(data, out[:wrote.value]) and np.array_equal(bb2, bb)
        tab = enc.last_launches()
        assert "k_vbs_plan<block_first>" in tab and "k_verify_frames<blocks>" in tab
        assert [x for x in tab if "k_vbs_plan" not in x and "k_verify_frames" not in x] == \
               [x for x in packed_list if "k_vbs_plan" not in x and "k_verify_frames" not in x]


def write_wav(path, pcm, bps, rate=44100):
    ch = pcm.shape[1]
    nb = (bps + 7) // 8
    raw = packed_bytes(pcm, bps)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * nb, ch * nb, bps) + b"data" +
                struct.pack("<I", len(raw)) + raw)


def test_cli_set_at_level_10_writes_the_single_input_files(tmp_path):
    cli = os.path.join(V.LIB_DIR, "flake_amd_cli")
    env = {k: v for k, v in os.environ.items() if k not in ("FLAKE_AMD_HOST_ASSEMBLY", "FLAKE_AMD_HOST_VBS")}
    r = _rng(31)
    outdir = tmp_path / "set"
    outdir.mkdir()
    wavs = []
    for i, lengths in enumerate(([4096] * 3 + [1000], [4096] * 2, [4096, 333])):
        pcm = np.concatenate(make_stream(r, lengths, 2, 16))
        w = tmp_path / f"in{i}.wav"
        write_wav(w, pcm, 16)
        wavs.append(str(w))
        one = subprocess.run([cli, "-10", str(w), str(tmp_path / f"single{i}.flac")], env=env, capture_output=True,
                             text=True, timeout=300)
        assert one.returncode == 0, one.stderr
    res = subprocess.run([cli, "-10", "--set", str(outdir), "--verify", *wavs], env=env, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr
    for i in range(len(wavs)):
        assert (tmp_path / f"single{i}.flac").read_bytes() == (outdir / f"in{i}.flac").read_bytes(), i


if __name__ == "__main__":
    import oraclelib
    byte_case(*CASES[int(sys.argv[1])], oraclelib.Oracle())
    print("case ok")
