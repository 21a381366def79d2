"""K7's segment mode (fhip_decode_frames_segments): the frames of several streams in one call, numbering, the size rule
and the strategy bit held per segment, placement for the batch as a whole, and the three per-segment outputs.  The
reference is fhip_decode_frames on each run alone and the PCM the frames were encoded from; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
import flacgen

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
V = flake_amd
SENT = -1234567


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def packed(enc, pcm, n, first=0):
    """fhip_encode_frames_packed: (stream bytes, frame sizes)."""
    pcm = np.ascontiguousarray(pcm, np.int32)
    nf = pcm.size // (n * enc.params.channels)
    fb = np.zeros(nf, np.int32)
    b = V.Batch()
    b.pcm, b.nframes, b.block_size = pcm.ctypes.data, nf, n
    b.frame_bytes, b.first_frame_number = fb.ctypes.data, first
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = C.c_int64(0)
    rc = enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), out.ctypes.data, cap, C.byref(wrote))
    assert rc == 0, enc.lib.fhip_last_error(enc._h)
    return out[:wrote.value].copy(), fb


def guarded(cap, ch, dtype=np.int32, guard=64):
    """(whole buffer, the [cap][ch] window inside it): sentinel rows before and after the output."""
    buf = np.full((cap + 2 * guard, ch), SENT if dtype == np.int32 else -1234, dtype)
    return buf, buf[guard:guard + cap]


def guards_intact(buf, cap, guard=64):
    s = buf.flat[0]
    return bool(np.all(buf[:guard] == s) and np.all(buf[guard + cap:] == s))


class Stream:
    """A stream of nf frames of n samples (and an optional shorter last one), numbered from `first`."""

    def __init__(self, enc, nf, n, first, seed, tail=0):
        ch, bps = enc.params.channels, enc.params.bits_per_sample
        self.pcm = flake_amd.synth_pcm(nf, n, ch, bps, first_frame=seed).reshape(-1, ch)
        self.s, self.fb = packed(enc, self.pcm, n, first)
        self.sizes = [n] * nf
        if tail:
            tp = flake_amd.synth_pcm(1, tail, ch, bps, first_frame=seed + 77).reshape(-1, ch)
            st, fbt = packed(enc, tp, tail, first + nf)
            self.s, self.fb, self.pcm = np.concatenate([self.s, st]), np.concatenate([self.fb, fbt]), np.concatenate([self.pcm, tp])
            self.sizes.append(tail)
        self.first = first
        self.off = np.concatenate([[0], np.cumsum(self.fb)])
        self.soff = np.concatenate([[0], np.cumsum(self.sizes)])

    def run(self, a, b):
        """(bytes, frame sizes, samples, number of the first frame) of frames a .. b."""
        return self.s[self.off[a]:self.off[b]], self.fb[a:b], self.pcm[self.soff[a]:self.soff[b]], self.first + a


def batch(runs):
    """runs -> (stream, frame_bytes, seg_first, seg_number, pcm, per-run sample counts)"""
    s = np.concatenate([r[0] for r in runs])
    fb = np.concatenate([r[1] for r in runs]).astype(np.int32)
    sf = np.concatenate([[0], np.cumsum([len(r[1]) for r in runs])]).astype(np.int32)
    num = np.array([r[3] for r in runs], np.int64)
    return s, fb, sf, num, np.concatenate([r[2] for r in runs]), [len(r[2]) for r in runs]


def seg_decode(enc, s, fb, cap, sf, num=None, var=None, **kw):
    buf, win = guarded(cap, enc.params.channels, enc.pcm_dtype)
    res = enc.decode_frames_segments(s, fb, cap, sf, num, var, out=win, **kw)
    assert guards_intact(buf, cap)
    return res


@pytest.fixture(scope="module")
def three():
    """Three streams of 64-sample stereo frames with different first numbers, and the five runs they are cut into."""
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        a, b, c = Stream(enc, 5, 64, 0, 1), Stream(enc, 5, 64, 100, 2), Stream(enc, 4, 64, 7, 3)
    return [a.run(0, 3), b.run(0, 2), a.run(3, 5), c.run(0, 4), b.run(2, 5)]


@pytest.mark.parametrize("fmt", ["int32", "int16"])
def test_five_segments_of_three_streams(three, fmt):
    s, fb, sf, num, pcm, counts = batch(three)
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        if fmt == "int16":
            enc.set_pcm_format(V.PCM_S16)
        alone = []
        for rs, rfb, rpcm, rnum in three:
            ok, out, ns, recs, summ, err = enc.decode_frames(rs, rfb, len(rpcm), False, rnum)
            assert ok and ns == len(rpcm), err
            alone.append(out[:ns].copy())
        alone = np.concatenate(alone)
        assert np.array_equal(alone, pcm.astype(enc.pcm_dtype))
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num)
        assert rc == V.OK, err
        assert enc.last_launches() == ["k_decode_frames segments", "k_decode", "k_decode_final", "k_decode_seg_final"]
        assert ns == len(pcm) and list(summ) == [len(fb), 0, -1, 0]
        assert out.dtype == alone.dtype and np.array_equal(out[:ns], alone)
        assert list(start) == list(np.cumsum([0] + counts[:-1])) and list(samples) == counts
        assert list(failed) == [-1] * 5
        assert np.all(recs["status"] == 0)
        # the same frames without the table: every boundary is a break in the numbering, and only that
        ok, _, _, recs, summ, _ = enc.decode_frames(s, fb, len(pcm), False, -1)
        assert not ok
        bad = np.flatnonzero(recs["status"])
        assert list(bad) == list(sf[1:-1])
        assert np.all(recs["status"][bad] == V.V_NUMBER) and np.all(recs["bit"][bad] == 32)


def message16(vals):
    return np.ascontiguousarray(vals.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :2].tobytes()


@pytest.mark.parametrize("fmt", ["int32", "int16"])
def test_segments_hashed_into_their_streams(three, torch, fmt):
    """The host form's md5 argument: K6 reads the ranges K7 left on the device; segments of one stream in batch order."""
    import hashlib
    s, fb, sf, num, pcm, counts = batch(three)
    seg_stream = [0, 1, 0, 2, 1]
    want = [hashlib.md5() for _ in range(4)]
    for (rs, rfb, rpcm, rnum), k in zip(three, seg_stream):
        want[k].update(message16(rpcm.reshape(-1)))
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        if fmt == "int16":
            enc.set_pcm_format(V.PCM_S16)
        states = torch.zeros(4 * V.MD5_STATE_BYTES, dtype=torch.uint8, device="cuda")
        digests = torch.zeros(4 * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.md5_init_dev(states, 4)
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num, md5_states=states,
                                                                          md5_nstreams=4, seg_stream=seg_stream)
        assert rc == V.OK and np.array_equal(out, pcm.astype(enc.pcm_dtype))
        tname = "int16_t" if fmt == "int16" else "int32_t"
        assert enc.last_launches() == ["k_decode_frames segments", "k_decode", "k_decode_final", "k_decode_seg_final",
                                       f"k_md5_ranges<{tname},2>"]
        enc.md5_final_dev(states, 4, digests)
        enc.sync()
        got = digests.cpu().numpy().reshape(4, 16)
        assert [got[k].tobytes() for k in range(4)] == [w.digest() for w in want]       # (stream 3 has no segment)
        bad = enc.decode_frames_segments(s, fb, len(pcm), sf, num, md5_states=states, md5_nstreams=4, seg_stream=[0, 1, 0, 4, 1])
        assert bad[0] == V.E_INVALID and enc.last_launches() == []


def test_seg_number_pins_the_first_frame(three):
    s, fb, sf, num, pcm, counts = batch(three)
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        good = seg_decode(enc, s, fb, len(pcm), sf, num)
        assert good[0] == V.OK
        wrong = num.copy()
        wrong[2] += 1
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, wrong)
        f = int(sf[2])
        assert rc == V.E_VERIFY and list(summ) == [len(fb), 1, f, V.V_NUMBER]
        assert list(np.flatnonzero(recs["status"])) == [f] and recs[f]["bit"] == 32
        assert list(failed) == [-1, -1, f, -1, -1]
        assert list(start) == list(good[5])                       # a misnumbered frame keeps its room ...
        assert list(samples) == [counts[0], counts[1], counts[2] - 64, counts[3], counts[4]] and ns == len(pcm) - 64
        keep = np.ones(len(pcm), bool)
        keep[start[2]:start[2] + 64] = False
        assert np.array_equal(out[keep], good[1][keep])           # ... and everything else is bit-identical
        # -1 accepts whatever the first frame carries
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, np.full(5, -1))
        assert rc == V.OK and np.array_equal(out, good[1]) and list(samples) == counts


def test_fixed_and_variable_segments_in_one_call():
    n = 256
    pv = P(10, block_size=n)
    si = V.HostStreaminfo(min_block_size=16, max_block_size=n, sample_rate=pv.sample_rate, channels=2, bits_per_sample=16)
    vpcm = np.ascontiguousarray(flake_amd.synth_pcm(3, n, 2, 16, first_frame=9), np.int32)
    with flake_amd.Encoder(pv, max_frames=64) as venc:
        cap = 8 * 3 * venc.frame_stride(n) + 64
        vs = np.zeros(cap, np.uint8)
        bb = np.zeros(3, np.int32)
        wrote, mx, nxt = C.c_int64(0), C.c_int(0), C.c_uint32(0)
        rc = venc.lib.fhip_encode_blocks_vbs_packed(venc._h, vpcm.ctypes.data, 3, n, 5 * n, vs.ctypes.data, cap,
                                                    bb.ctypes.data, None, C.byref(wrote), C.byref(mx), C.byref(nxt))
        assert rc == 0
        vs = vs[:wrote.value].copy()
    vfb, used = V.index_frames(si, vs)
    assert used == len(vs) and len(vfb) >= 3
    with flake_amd.Encoder(P(5, block_size=n, variable_block_size=0), max_frames=64) as enc:
        a = Stream(enc, 3, n, 4, 5, tail=100)
        runs = [a.run(0, 4), (vs, np.asarray(vfb, np.int32), vpcm.reshape(-1, 2), 5 * n)]
        s, fb, sf, num, pcm, counts = batch(runs)
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num, [0, 1])
        assert rc == V.OK, err
        assert np.array_equal(out, pcm) and list(samples) == counts and list(start) == [0, counts[0]]
        # the wrong strategy for the second segment: HEADER on each of its frames, none of which takes room
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num, [0, 0])
        assert rc == V.E_VERIFY and np.all(recs["status"][:4] == 0) and np.all(recs["status"][4:] == V.V_HEADER)
        assert list(failed) == [-1, 4] and list(samples) == [counts[0], 0] and ns == counts[0]
        assert np.array_equal(out[:ns], pcm[:ns])
        # ... and for the first
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num, [1, 1])
        assert rc == V.E_VERIFY and np.all(recs["status"][:4] == V.V_HEADER) and np.all(recs["status"][4:] == 0)
        assert list(failed) == [0, -1] and list(samples) == [0, counts[1]] and list(start) == [0, 0]
        assert np.array_equal(out[:ns], pcm[counts[0]:])


def test_short_frames_inside_and_at_the_end_of_a_segment():
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        a, b = Stream(enc, 3, 64, 0, 1, tail=40), Stream(enc, 2, 64, 50, 2)
        # a's short last frame ends segment 0; b follows
        s, fb, sf, num, pcm, counts = batch([a.run(0, 4), b.run(0, 2)])
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num)
        assert rc == V.OK and np.array_equal(out, pcm) and list(samples) == [3 * 64 + 40, 128]
        # the same short frame with frames of its own segment behind it
        short, fbs = packed(enc, flake_amd.synth_pcm(1, 40, 2, 16, first_frame=31), 40, 2)
        c = Stream(enc, 4, 64, 0, 4)
        s2 = np.concatenate([c.s[:c.off[2]], short, c.s[c.off[3]:], b.s])
        fb2 = np.concatenate([c.fb[:2], fbs, c.fb[3:], b.fb]).astype(np.int32)
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s2, fb2, 6 * 64, [0, 4, 6], [0, 50])
        assert rc == V.E_VERIFY and recs[2]["status"] == V.V_NUMBER and recs[2]["bit"] == 16
        assert list(failed) == [2, -1] and np.all(recs["status"][[0, 1, 4, 5]] == 0)
        assert np.array_equal(out[start[1]:start[1] + 128], b.pcm)


def test_segment_boundaries_around_the_header_pass_chunk():
    """1100 mono frames of 16 samples; segments end at frames 1023, 1024 and 1025: the carry from the pass's first 1024
    frames must not bind a segment's first frame to the frame before it."""
    p = P(5, channels=1, block_size=16, variable_block_size=0)
    with flake_amd.Encoder(p, max_frames=1100) as enc:
        st = [Stream(enc, 1023, 16, 3, 1), Stream(enc, 1, 16, 900, 2), Stream(enc, 1, 16, 0, 3), Stream(enc, 75, 16, 40, 4)]
        runs = [x.run(0, len(x.fb)) for x in st]
        s, fb, sf, num, pcm, counts = batch(runs)
        assert list(sf) == [0, 1023, 1024, 1025, 1100]
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), sf, num)
        assert rc == V.OK, err
        assert np.array_equal(out, pcm) and list(samples) == counts and list(failed) == [-1] * 4
        assert list(start) == [0, 1023 * 16, 1024 * 16, 1025 * 16]
        # with the boundaries one frame off, the numbering breaks where the streams really change
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, len(pcm), [0, 1022, 1024, 1026, 1100],
                                                                          [3, 3 + 1022, 0, 41])
        assert rc == V.E_VERIFY and list(np.flatnonzero(recs["status"])) == [1023, 1025]
        assert list(failed) == [-1, 1023, 1025, -1]


def utf8_len(b0):
    """Bytes of the coded number whose first byte is b0."""
    n = 0
    while (b0 << n) & 0x80:
        n += 1
    return max(n, 1)


def test_broken_header_and_late_failure(three):
    s, fb, sf, num, pcm, counts = batch(three[:3])
    off = np.concatenate([[0], np.cumsum(fb)])
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        good = seg_decode(enc, s, fb, len(pcm), sf, num)
        assert good[0] == V.OK
        bad = s.copy()
        f = int(sf[1])                                         # the first frame of segment 1: a bit of its header's CRC-8
        fr = s[off[f]:off[f + 1]]
        p = 4 + utf8_len(int(fr[4])) + {6: 1, 7: 2}.get(int(fr[2]) >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(int(fr[2]) & 15, 0)
        assert flacgen.crc8(bytes(fr[:p])) == fr[p]            # (that byte is the CRC-8)
        bad[off[f] + p] ^= 0x10
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, bad, fb, len(pcm), sf, num)
        assert rc == V.E_VERIFY and recs[f]["status"] == V.V_CRC8 and list(np.flatnonzero(recs["status"])) == [f]
        assert list(failed) == [-1, f, -1]
        assert list(start) == [0, counts[0], counts[0] + counts[1] - 64]       # it takes no room
        assert list(samples) == [counts[0], counts[1] - 64, counts[2]] and ns == len(pcm) - 64
        assert np.array_equal(out[:counts[0]], pcm[:counts[0]])
        assert np.array_equal(out[start[1]:start[1] + 64], pcm[counts[0] + 64:counts[0] + 128])
        assert np.array_equal(out[start[2]:start[2] + counts[2]], pcm[counts[0] + counts[1]:])
        # a failure that only k_decode finds: the CRC-16 of the last frame of segment 2
        late = s.copy()
        g = len(fb) - 1
        late[off[g + 1] - 1] ^= 0x01
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, late, fb, len(pcm), sf, num)
        assert rc == V.E_VERIFY and recs[g]["status"] == V.V_CRC16 and list(failed) == [-1, -1, g]
        assert list(samples) == counts and ns == len(pcm)       # placed and counted; its own range is unspecified
        assert np.array_equal(out[:len(pcm) - 64], pcm[:len(pcm) - 64])


@pytest.mark.parametrize("fmt", ["int32", "int16"])
def test_pcm_cap_one_sample_short(three, fmt):
    s, fb, sf, num, pcm, counts = batch(three)
    cap = len(pcm) - 1
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        if fmt == "int16":
            enc.set_pcm_format(V.PCM_S16)
        rc, out, ns, recs, summ, start, samples, failed, err = seg_decode(enc, s, fb, cap, sf, num)   # (checks the guards)
        last = len(fb) - 1
        assert rc == V.E_VERIFY and list(summ) == [len(fb), 1, last, V.V_NUMBER] and recs[last]["bit"] == 16
        assert ns == len(pcm) - 64 and list(samples) == counts[:4] + [counts[4] - 64] and list(failed) == [-1] * 4 + [last]
        assert np.array_equal(out[:ns], pcm[:ns].astype(enc.pcm_dtype))


def test_invalid_tables_queue_nothing(three):
    s, fb, sf, num, pcm, counts = batch(three)
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        assert seg_decode(enc, s, fb, len(pcm), sf, num)[0] == V.OK and enc.last_launches()
        for bad_sf, bad_num in (([0, 5, 3, 7, 11, len(fb)], num), ([0, 3, 5, 7, 11, len(fb) - 1], num),
                                ([0, 3, 5, 7, 11, len(fb) + 1], num), ([1, 3, 5, 7, 11, len(fb)], num), ([0], num[:1])):
            res = enc.decode_frames_segments(s, fb, len(pcm), bad_sf, bad_num)
            assert res[0] == V.E_INVALID, bad_sf
            assert enc.last_launches() == []
            assert np.all(res[1] == 0) and np.all(res[5] == -7)          # nothing came back
        for var in ([0, 0, 2, 0, 0],):
            assert enc.decode_frames_segments(s, fb, len(pcm), sf, num, var)[0] == V.E_INVALID
            assert enc.last_launches() == []


def test_no_table_is_the_existing_entry():
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        a = Stream(enc, 6, 64, 0, 1, tail=33)
        for stream in (a.s, np.concatenate([a.s[:a.off[2]], a.s[a.off[3]:]])):       # good, and with a gap in the numbers
            fb = a.fb if len(stream) == len(a.s) else np.concatenate([a.fb[:2], a.fb[3:]])
            cap = len(a.pcm)
            ok, out, ns, recs, summ, err = enc.decode_frames(stream, fb, cap, False, -1)
            want_l = enc.last_launches()
            rc, out2, ns2, recs2, summ2, _, _, _, err2 = enc.decode_frames_segments(stream, fb, cap, [0, len(fb)],
                                                                                    use_segments=False)
            assert enc.last_launches() == want_l == ["k_decode_frames", "k_decode", "k_decode_final"]
            assert (rc == V.OK) == ok and ns2 == ns and err2 == err
            assert out2.tobytes() == out.tobytes() and recs2.tobytes() == recs.tobytes() and list(summ2) == list(summ)
