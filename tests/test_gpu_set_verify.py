"""K5's numbered mode and verification of stream sets: every frame of a batch is held to a number table, whichever
stream owns it (fhip_verify_frames_numbered*, fhip_set_verify on batches with fhip_batch.frame_numbers,
flake_amd_set_enable_verify, flake_amd_cli --set --verify).

The path on which flake_amd_set_encode returns -1 and flake_amd_set_last_verify_failure is filled cannot be reached
from outside without breaking the encoder, and no switch exists to force it.  It is covered by the C-ABI cases
below, which exercise the verdict (first failing batch index, status, subframe, sample, bit) that the host layer
relays, and by review of the mapping from batch index to stream and frame number in flake_set.c."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import flake_amd
from cases import _rng

pytestmark = pytest.mark.gpu

V = flake_amd
P = flake_amd.level_params
K5 = ["k_verify_frames", "k_verify", "k_verify_final"]

# every UTF-8 length of a frame number and every length boundary, out of order
NUMBERS = [5, 0, 127, 128, 2047, 2048, 65535, 65536, 2 ** 21 - 1, 2 ** 21, 2 ** 26, 2 ** 31 - 1]


def packed(enc, pcm, n, numbers=None, first=0):
    """fhip_encode_frames_packed with an optional frame number table: (rc, stream bytes, frame sizes)."""
    pcm = np.ascontiguousarray(pcm, enc.pcm_dtype)
    nf = pcm.size // (n * enc.params.channels)
    fb = np.zeros(nf, np.int32)
    b = V.Batch()
    b.pcm, b.nframes, b.block_size = pcm.ctypes.data, nf, n
    b.frame_bytes, b.first_frame_number = fb.ctypes.data, first
    nums = None
    if numbers is not None:
        nums = np.ascontiguousarray(numbers, np.uint32)
        assert len(nums) == nf
        b.frame_numbers = nums.ctypes.data
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = C.c_int64(0)
    rc = enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), out.ctypes.data, cap, C.byref(wrote))
    return rc, out[:wrote.value].copy(), fb


def numbered_raw(enc, stream, fb, pcm, numbers, first=0):
    """fhip_verify_frames_numbered itself (a None table goes to the entry as NULL): (rc, records, summary)."""
    st = np.ascontiguousarray(stream, np.uint8)
    fb = np.ascontiguousarray(fb, np.int32)
    pc = np.ascontiguousarray(pcm, enc.pcm_dtype).reshape(-1, enc.params.channels)
    nums = None if numbers is None else np.ascontiguousarray(numbers, np.uint32)
    recs = np.zeros(len(fb), V.VERIFY_REC_DTYPE)
    summ = np.zeros(4, np.int64)
    vi = V.VerifyIn(st.ctypes.data, st.size, fb.ctypes.data, len(fb), pc.ctypes.data, pc.shape[0], first)
    vo = V.VerifyOut(recs.ctypes.data, summ.ctypes.data)
    rc = enc.lib.fhip_verify_frames_numbered(enc._h, C.byref(vi), None if nums is None else nums.ctypes.data,
                                             C.byref(vo))
    return rc, recs, summ


def err(enc):
    return enc.lib.fhip_last_error(enc._h).decode()


@pytest.fixture(scope="module")
def batch12():
    """Level 2, stereo 16-bit, 12 frames of 1152: the bytes with verification off, numbered by NUMBERS."""
    p = P(2)
    n = p.block_size
    assert n == 1152
    pcm = V.synth_pcm(12, n, 2, 16)
    with V.Encoder(p, max_frames=12) as enc:
        rc, s, fb = packed(enc, pcm, n, NUMBERS)
        assert rc == 0, err(enc)
    return p, n, pcm, s, fb


# ---- through the C ABI ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [V.PCM_S32, V.PCM_S16], ids=["s32", "s16"])
def test_explicit_numbers_under_set_verify(batch12, fmt):
    """An out-of-order table with verification on: FHIP_OK and the verification-off bytes, at both PCM widths.
    (Before the numbered mode the verifier took frame_numbers[0] as the origin of a sequence: NUMBER.)"""
    p, n, pcm, s0, fb0 = batch12
    with V.Encoder(p, max_frames=12) as enc:
        enc.set_pcm_format(fmt)
        enc.set_verify(True)
        rc, s1, fb1 = packed(enc, pcm, n, NUMBERS)
        assert rc == V.OK, (rc, err(enc))
        assert np.array_equal(s1, s0) and np.array_equal(fb1, fb0)
        # the same verdicts from the caller's entry at this width
        ok, recs, summ, msg = enc.verify_frames(s1, fb1, pcm, frame_numbers=NUMBERS)
        assert ok, msg
        assert np.all(recs["status"] == V.V_OK) and list(summ) == [12, 0, -1, 0]


def test_numbered_host_entry_clean(batch12):
    p, n, pcm, s, fb = batch12
    with V.Encoder(p, max_frames=12) as enc:
        ok, recs, summ, msg = enc.verify_frames(s, fb, pcm, frame_numbers=NUMBERS)
        assert ok, msg
        assert np.all(recs["status"] == V.V_OK) and np.all(recs["bit"] == -1)
        assert list(summ) == [12, 0, -1, 0]
        # a NULL table is fhip_verify_frames: the same records, element for element, failures included
        rc, s2, fb2 = packed(enc, pcm, n, first=7)
        assert rc == 0
        bad = pcm.reshape(-1, 2).copy()
        bad[5 * n + 33, 1] += 3
        for x, want_rc in ((pcm, V.OK), (bad, V.E_VERIFY)):
            ok, r_old, sum_old, _ = enc.verify_frames(s2, fb2, x, first_sample=7 * n)
            rc, r_new, sum_new = numbered_raw(enc, s2, fb2, x, None, first=7 * n)
            assert rc == want_rc and ok == (want_rc == V.OK)
            assert np.array_equal(r_old, r_new) and np.array_equal(sum_old, sum_new)
        assert list(np.nonzero(r_new["status"])[0]) == [5]


@pytest.mark.parametrize("f,how", [(4, "plus1"), (7, "other"), (0, "plus1"), (11, "other")])
def test_wrong_number_fails_exactly_that_frame(batch12, f, how):
    p, n, pcm, s, fb = batch12
    nums = list(NUMBERS)
    nums[f] = nums[f] + 1 if how == "plus1" else NUMBERS[(f + 5) % 12]
    assert nums[f] != NUMBERS[f]
    with V.Encoder(p, max_frames=12) as enc:
        ok, recs, summ, msg = enc.verify_frames(s, fb, pcm, frame_numbers=nums)
        assert not ok
        assert list(np.nonzero(recs["status"])[0]) == [f]
        assert recs[f]["status"] == V.V_NUMBER and recs[f]["bit"] == 32
        assert list(summ) == [12, 1, f, V.V_NUMBER]
        assert "NUMBER" in msg and f"number {nums[f]}" in msg, msg
        s4, r4 = np.zeros(4, np.int64), np.zeros(1, V.VERIFY_REC_DTYPE)
        assert enc.lib.fhip_last_verify_failure(enc._h, s4.ctypes.data, r4.ctypes.data) == 1
        assert list(s4) == list(summ) and r4[0] == recs[f]


def test_two_streams_frames_exchanged():
    """Slots 2 and 3 both carry number 1 (one of each stream): with their bytes exchanged the framing, the CRCs
    and the numbers all stay valid, and only the content can tell."""
    p = P(2)
    n = p.block_size
    a, b = V.synth_pcm(6, n, 2, 16, first_frame=0), V.synth_pcm(6, n, 2, 16, first_frame=31)
    pcm = np.stack([a, b], axis=1).reshape(12, n, 2)
    nums = [k // 2 for k in range(12)]
    assert nums[2] == nums[3] == 1
    with V.Encoder(p, max_frames=12) as enc:
        enc.set_verify(True)
        rc, s, fb = packed(enc, pcm, n, nums)
        assert rc == 0, err(enc)
        off = np.concatenate([[0], np.cumsum(fb)])
        fr = [s[off[k]:off[k + 1]] for k in range(12)]
        assert fr[2].tobytes() != fr[3].tobytes()
        fr[2], fr[3] = fr[3], fr[2]
        ok, recs, summ, msg = enc.verify_frames(np.concatenate(fr), [len(q) for q in fr], pcm, frame_numbers=nums)
        assert not ok
        assert list(np.nonzero(recs["status"])[0]) == [2, 3], recs
        for k in (2, 3):
            assert recs[k]["status"] not in (V.V_NUMBER, V.V_HEADER, V.V_CRC8), recs[k]
        assert summ[1] == 2 and summ[2] == 2


def test_short_blocks():
    """A tail call: 5 frames of 333 samples on block-4096 parameters, each the end of a stream of its own."""
    p = P(5)
    assert p.block_size == 4096
    t = 333
    pcm = V.synth_pcm(5, t, 2, 16, first_frame=3)
    nums = [9, 0, 77, 300, 4]
    with V.Encoder(p, max_frames=8) as enc:
        rc, s0, fb0 = packed(enc, pcm, t, nums)
        assert rc == 0
        enc.set_verify(True)
        rc, s, fb = packed(enc, pcm, t, nums)
        assert rc == V.OK, err(enc)
        assert np.array_equal(s, s0) and np.array_equal(fb, fb0)
    # the caller's entry takes the handle's block size as the frames' length
    with V.Encoder(P(5, block_size=t, max_partition_order=0), max_frames=8) as enc:
        ok, recs, summ, msg = enc.verify_frames(s, fb, pcm, frame_numbers=nums)
        assert ok, msg
    # ... so 334 samples of PCM per frame is this test's own mis-slicing: no frame holds 334 samples
    wide = np.concatenate([pcm, pcm[:, :1]], axis=1)
    assert wide.shape == (5, t + 1, 2)
    with V.Encoder(P(5, block_size=t + 1, max_partition_order=0), max_frames=8) as enc:
        ok, recs, summ, msg = enc.verify_frames(s, fb, wide, frame_numbers=nums)
        assert not ok
        assert np.all(recs["status"] == V.V_NUMBER) and np.all(recs["bit"] == 16), recs
        assert list(summ) == [5, 5, 0, V.V_NUMBER]


def test_more_than_one_header_chunk():
    """1030 frames cross the 1024-frame loop of k_verify_frames; two interleaved streams."""
    p = P(0, channels=1, block_size=256)
    n, nf = 256, 1030
    pcm = V.synth_pcm(nf, n, 1, 16, first_frame=2)
    nums = np.array([f // 2 if f % 2 == 0 else 70000 + f // 2 for f in range(nf)], np.uint32)
    with V.Encoder(p, max_frames=nf) as enc:
        enc.set_verify(True)
        rc, s, fb = packed(enc, pcm, n, nums)
        assert rc == V.OK, err(enc)
        ok, recs, summ, msg = enc.verify_frames(s, fb, pcm, frame_numbers=nums)
        assert ok and list(summ) == [nf, 0, -1, 0], msg
        bad = nums.copy()
        bad[1025] += 1
        ok, recs, summ, msg = enc.verify_frames(s, fb, pcm, frame_numbers=bad)
        assert not ok
        assert list(np.nonzero(recs["status"])[0]) == [1025]
        assert recs[1025]["status"] == V.V_NUMBER and recs[1025]["bit"] == 32
        assert list(summ) == [nf, 1, 1025, V.V_NUMBER]


def test_table_refused_on_a_vbs_handle(batch12):
    _, n, pcm, s, fb = batch12
    p = P(10)
    assert p.allow_vbs
    with V.Encoder(p, max_frames=16) as enc:
        before = enc.last_launches()
        rc, recs, summ = numbered_raw(enc, s, fb, pcm, NUMBERS)
        assert rc == V.E_UNSUPPORTED
        assert "fixed-block" in err(enc)
        assert enc.last_launches() == before
        assert list(summ) == [0, 0, 0, 0] and not recs["status"].any()      # nothing ran, nothing was written
        dummy = np.zeros(4, np.int64)
        vi = V.VerifyIn(s.ctypes.data, s.size, fb.ctypes.data, len(fb), pcm.ctypes.data, 12 * n, 0)
        vo = V.VerifyOut(None, dummy.ctypes.data)
        nums = np.array(NUMBERS, np.uint32)
        # (refused before any pointer is looked at: these are host addresses)
        assert enc.lib.fhip_verify_frames_numbered_dev(enc._h, C.byref(vi), nums.ctypes.data,
                                                       C.byref(vo)) == V.E_UNSUPPORTED
        assert enc.last_launches() == before


def test_off_means_off(batch12):
    p, n, pcm, s, fb = batch12
    with V.Encoder(p, max_frames=12) as enc:
        rc, _, _ = packed(enc, pcm, n, NUMBERS)
        assert rc == 0
        off = enc.last_launches()
        assert off and not [x for x in off if x.startswith("k_verify")]
        enc.set_verify(True)
        rc, _, _ = packed(enc, pcm, n, NUMBERS)
        assert rc == 0, err(enc)
        on = enc.last_launches()
        assert [x for x in on if x.startswith("k_verify")] == K5
        assert [x for x in on if not x.startswith("k_verify")] == off
        enc.set_verify(False)
        rc, _, _ = packed(enc, pcm, n, NUMBERS)
        assert rc == 0 and enc.last_launches() == off


# ---- the host layer ------------------------------------------------------------------------------------
# (make_streams / run_set: local copies of test_gpu_stream_set.py's, which is not imported so that it is not
# collected a second time)

def make_streams(r, nstreams, bs, ch, bits, max_blocks):
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


def run_set(st, streams, bs, dtype, r, ncalls=3):
    got = [bytearray() for _ in streams]
    todo = [(k, s) for s, p in enumerate(streams) for k in range(p.shape[0] // bs)]
    todo.sort()
    cuts = sorted(set([0, len(todo)] + [int(x) for x in r.randint(0, len(todo) + 1, ncalls - 1)]))
    for c, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        part = todo[a:b]
        if c % 2:
            queues = {}
            for k, s in part:
                queues.setdefault(s, []).append(k)
            lanes = [s for s, q in queues.items() for _ in q]
            r.shuffle(lanes)
            part = [(queues[s].pop(0), s) for s in lanes]
        pcm = np.concatenate([streams[s][k * bs:(k + 1) * bs] for k, s in part])
        data, sizes = st.encode(pcm, bs, [s for _, s in part], dtype=dtype)
        assert st.last_verify_failure() is None
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
        assert st.last_verify_failure() is None
        pos = 0
        for s, fs in zip(members, sizes):
            got[s] += data[pos:pos + fs].tobytes()
            pos += fs
    return [bytes(g) for g in got], tails


def set_outputs(nstreams, level, ch, bits, dtype, max_blocks, verify, flags=0, seed=None):
    """(per-stream bytes, STREAMINFO bytes, tails) of one seeded run; st.encode raises when a call fails."""
    r = _rng(nstreams * 100 + level * 10 + ch + bits if seed is None else seed)
    with V.StreamSet(nstreams, level=level, channels=ch, bits_per_sample=bits, flags=flags) as st:
        assert st.last_verify_failure() is None
        if verify:
            st.set_verify(True)
        streams = make_streams(r, nstreams, st.block_size, ch, bits, max_blocks)
        got, tails = run_set(st, streams, st.block_size, dtype, r)
        infos = [st.streaminfo_bytes(s) for s in range(nstreams)]
        assert st.last_verify_failure() is None
    return got, infos, tails


@pytest.mark.parametrize("nstreams,level,ch,bits,dtype,max_blocks", [
    (17, 8, 2, 16, np.int16, 6), (17, 5, 2, 24, np.int32, 6), (2, 2, 8, 16, np.int16, 5)])
def test_set_bytes_unchanged(nstreams, level, ch, bits, dtype, max_blocks):
    off = set_outputs(nstreams, level, ch, bits, dtype, max_blocks, False)
    on = set_outputs(nstreams, level, ch, bits, dtype, max_blocks, True)
    assert on[0] == off[0] and on[1] == off[1]
    tails = on[2]
    assert sum(len(g) for g in on[0]) > 0
    assert any(len(m) > 1 for m in tails.values()) or nstreams == 2      # grouped tails were verified too


def test_set_md5_modes():
    outs = {}
    for flags in (0, V.SET_MD5_HOST, V.SET_MD5_OFF):
        for verify in (False, True):
            got, infos, _ = set_outputs(9, 2, 2, 16, np.int16, 7, verify, flags=flags, seed=4)
            outs[flags, verify] = (got, infos)
        assert outs[flags, True] == outs[flags, False], flags
    assert outs[0, True] == outs[V.SET_MD5_HOST, True]
    assert outs[V.SET_MD5_OFF, True][0] == outs[0, True][0]
    for s in range(9):
        assert outs[V.SET_MD5_OFF, True][1][s][18:] == bytes(16)
        assert outs[0, True][1][s][18:] != bytes(16)


def test_set_verify_null_set():
    lib = V.load_host_library()
    assert lib.flake_amd_set_enable_verify(None, 1) == -1
    assert lib.flake_amd_set_last_verify_failure(None, None, None, None) == 0


def write_wav(path, pcm, bps, rate=44100):
    ch = pcm.shape[1]
    nb = (bps + 7) // 8
    raw = np.ascontiguousarray(pcm.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * nb, ch * nb, bps) + b"data" +
                struct.pack("<I", len(raw)) + raw)


def test_cli_set_verify(tmp_path):
    cli = os.path.join(V.LIB_DIR, "flake_amd_cli")
    env = {k: v for k, v in os.environ.items() if k not in ("FLAKE_AMD_HOST_ASSEMBLY", "FLAKE_AMD_HOST_VBS")}
    lengths = (4096 * 5 + 1234, 4096 * 2, 4096 * 7 + 1234)
    wavs = []
    for i, n in enumerate(lengths):
        pcm = V.synth_pcm(8, 4096, 2, 16, first_frame=11 * i).reshape(-1, 2)[:n]
        w = tmp_path / f"in{i}.wav"
        write_wav(w, pcm, 16)
        wavs.append(str(w))
    for name, extra in (("plain", []), ("checked", ["--verify"])):
        (tmp_path / name).mkdir()
        r = subprocess.run([cli, "-5", "--set", str(tmp_path / name), *extra, *wavs], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    for i in range(len(lengths)):
        a = (tmp_path / "plain" / f"in{i}.flac").read_bytes()
        b = (tmp_path / "checked" / f"in{i}.flac").read_bytes()
        assert len(a) > 1000 and a == b, i
    assert sorted(os.listdir(tmp_path / "checked")) == ["in0.flac", "in1.flac", "in2.flac"]
