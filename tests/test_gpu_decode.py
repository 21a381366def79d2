"""K7, the on-device decoder (fhip_decode_frames, fhip_decode_frames_dev): every form of the format against a
hand-written frame writer and the CPU test decoder, round trips of this encoder's own output, the bit reader's
corners, and corrupt streams, which must end in a status code.  Every comparison is exact integer equality."""
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


def vbs_packed(enc, pcm, nblocks, n, first=0):
    pcm = np.ascontiguousarray(pcm, np.int32)
    cap = 8 * nblocks * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    bb = np.zeros(nblocks, np.int32)
    wrote = C.c_int64(0)
    mx, nxt = C.c_int(0), C.c_uint32(0)
    rc = enc.lib.fhip_encode_blocks_vbs_packed(enc._h, pcm.ctypes.data, nblocks, n, first, out.ctypes.data, cap,
                                               bb.ctypes.data, None, C.byref(wrote), C.byref(mx), C.byref(nxt))
    assert rc == 0, enc.lib.fhip_last_error(enc._h)
    return out[:wrote.value].copy()


def guarded(cap, ch, dtype=np.int32, guard=64):
    """(whole buffer, the [cap][ch] window inside it): sentinel rows before and after the output."""
    buf = np.full((cap + 2 * guard, ch), SENT if dtype == np.int32 else -1234, dtype)
    return buf, buf[guard:guard + cap]


def guards_intact(buf, cap, guard=64):
    s = buf.flat[0]
    return bool(np.all(buf[:guard] == s) and np.all(buf[guard + cap:] == s))


def decode_ok(enc, stream, fb, want, vb=False, first=-1):
    """Decode through the host entry into a guarded buffer of exactly the samples wanted; everything must be right."""
    want = np.asarray(want).reshape(-1, enc.params.channels)
    cap = want.shape[0]
    buf, win = guarded(cap, enc.params.channels, enc.pcm_dtype)
    ok, out, ns, recs, summ, err = enc.decode_frames(stream, fb, cap, vb, first, out=win)
    assert ok, (err, recs[recs["status"] != 0][:4])
    assert ns == cap
    assert list(summ) == [len(fb), 0, -1, 0]
    assert np.all(recs["status"] == 0) and np.all(recs["bit"] == -1)
    assert np.array_equal(out[:ns], want.astype(enc.pcm_dtype))
    assert guards_intact(buf, cap)
    return out


# ---- 1. every form -------------------------------------------------------------------------------

def extra_forms():
    """A 33-bit side channel (32-bit stereo, each side mode) and eight channels."""
    out = []
    st = [dict(kind="fixed", order=2, porder=2), dict(kind="fixed", order=1, porder=2)]
    x = flacgen.test_signal(192, 2, 32, seed=21)
    for cc in (8, 9, 10):
        out.append((f"ch{cc}_32bit", x, flacgen.frame(x, 0, 32, 44100, st, ch_code=cc), 32, 44100, 2))
    out.append(("ch10_32bit_verbatim_side", x, flacgen.frame(x, 0, 32, 44100, [st[0], dict(kind="verbatim")], ch_code=10),
                32, 44100, 2))
    y = flacgen.test_signal(256, 8, 16, seed=22)
    subs = [dict(kind="fixed", order=c % 5, porder=c % 3) for c in range(6)] + [dict(kind="verbatim"),
                                                                               dict(kind="lpc", order=3, coefs=[3, -3, 1],
                                                                                    precision=4, shift=0, porder=1)]
    out.append(("eight_channels", y, flacgen.frame(y, 0, 16, 44100, subs), 16, 44100, 8))
    return out


FORMS = {}


def forms(key):
    if key not in FORMS:
        FORMS[key] = flacgen.catalogue(bps=key) if key in (16, 24) else extra_forms()
    return FORMS[key]


@pytest.mark.parametrize("key", [16, 24, "extra"])
def test_every_form(decoder, key):
    for name, pcm, fr, bps, sr, nch in forms(key):
        p = P(5, channels=nch, bits_per_sample=bps, sample_rate=sr, block_size=max(len(pcm), 16))
        ref, _ = decoder.decode(np.frombuffer(fr, np.uint8), nch, bps, len(pcm))
        assert np.array_equal(ref, pcm), name                        # the two CPU answers agree
        with flake_amd.Encoder(p, max_frames=2) as enc:
            decode_ok(enc, np.frombuffer(fr, np.uint8), [len(fr)], pcm, vb=False, first=0)


def test_long_numbers_variable_blocks(decoder):
    for first, pcm, fr in flacgen.utf8_catalogue():
        with flake_amd.Encoder(P(5, channels=1, block_size=4096), max_frames=2) as enc:
            decode_ok(enc, np.frombuffer(fr, np.uint8), [len(fr)], pcm, vb=True, first=first)
            decode_ok(enc, np.frombuffer(fr, np.uint8), [len(fr)], pcm, vb=True, first=-1)
            # the wrong strategy bit or the wrong first number is a status, not a decode
            ok, _, ns, recs, summ, _ = enc.decode_frames(fr, [len(fr)], len(pcm), False, -1)
            assert not ok and recs[0]["status"] == V.V_HEADER and ns == 0
            ok, _, ns, recs, summ, _ = enc.decode_frames(fr, [len(fr)], len(pcm), True, first + 1)
            assert not ok and recs[0]["status"] == V.V_NUMBER and ns == 0


# ---- 2. bit-reader corners -----------------------------------------------------------------------

def unzig(u):
    return u >> 1 if u % 2 == 0 else -((u + 1) >> 1)


def corner_frames():
    n = 192
    out = []
    # parameter 0: the residual's zig-zag value is its unary run
    x = np.zeros((n, 1), np.int32)
    runs = [31, 32, 33, 63, 64, 65, 200]
    for i, r in enumerate(runs):
        x[5 + 11 * i, 0] = unzig(r)
    x[190, 0] = unzig(200)
    out.append(("unary_runs", x, 16, [dict(kind="fixed", order=0, porder=0, ks=[0])]))
    # the same runs against a prediction (FIXED 1: the residual is the difference)
    out.append(("unary_runs_fixed1", np.cumsum(x, axis=0).astype(np.int32), 16, [dict(kind="fixed", order=1, porder=0, ks=[0])]))
    out.append(("rice2_k30", flacgen.test_signal(n, 1, 24, seed=31), 24, [dict(kind="fixed", order=0, method=1, porder=0, ks=[30])]))
    # the block's largest partition order: three samples per partition, the first holds one residual
    out.append(("porder6_fixed2", flacgen.test_signal(n, 1, 16, seed=32), 16, [dict(kind="fixed", order=2, porder=6)]))
    # an escape partition of raw width 0 directly before one of width 31
    z = np.zeros((n, 1), np.int32)
    z[96:, 0] = np.where(np.arange(96) % 2, (1 << 30) - 1, -(1 << 30))
    out.append(("escape_0_then_31", z, 32, [dict(kind="fixed", order=0, porder=1, escape=(0, 1))]))
    # FIXED 0, parameter 3: 66 + 192 * 4 bits before the quotients; m samples with quotient 1 add m bits
    for m, nbytes in ((6, 107), (7, 108)):
        w = np.full((n, 1), 2, np.int32)
        w[:m, 0] = 5                                             # zig-zag 10: quotient 1
        out.append((f"padding_{(8 - (834 + m) % 8) % 8}", w, 16, [dict(kind="fixed", order=0, porder=0, ks=[3])], nbytes))
    return out


def test_bit_reader_corners(decoder):
    for name, pcm, bps, subs, *rest in corner_frames():
        fr = flacgen.frame(pcm, 0, bps, 44100, subs)
        if rest:
            assert len(fr) == rest[0], (name, len(fr))              # 0 and 7 padding bits, as constructed
        ref, _ = decoder.decode(np.frombuffer(fr, np.uint8), 1, bps, len(pcm))
        assert np.array_equal(ref, pcm), name
        with flake_amd.Encoder(P(5, channels=1, bits_per_sample=bps, block_size=192), max_frames=2) as enc:
            decode_ok(enc, np.frombuffer(fr, np.uint8), [len(fr)], pcm, first=0)


def test_escape_widths_are_what_the_case_says():
    name, pcm, bps, subs = corner_frames()[4]
    assert flacgen.minbits_signed([int(v) for v in pcm[:96, 0]]) == 0
    assert flacgen.minbits_signed([int(v) for v in pcm[96:, 0]]) == 31


# ---- 3. round trips of this encoder's own output ---------------------------------------------------

def roundtrip(p, n, nframes, first=0, first_number=None, tail=0, pcm=None, seed=0):
    p = p.copy()
    p.block_size = n
    ch = p.channels
    if pcm is None:
        pcm = flake_amd.synth_pcm(nframes, n, ch, p.bits_per_sample, first_frame=seed)
    pcm = np.ascontiguousarray(pcm, np.int32).reshape(-1, ch)
    with flake_amd.Encoder(p, max_frames=nframes + 1) as enc:
        s, fb = packed(enc, pcm, n, first)
        if tail:
            tp = flake_amd.synth_pcm(1, tail, ch, p.bits_per_sample, first_frame=seed + 99).reshape(-1, ch)
            st, fbt = packed(enc, tp, tail, first + nframes)
            s, fb, pcm = np.concatenate([s, st]), np.concatenate([fb, fbt]), np.concatenate([pcm, tp])
        decode_ok(enc, s, fb, pcm, vb=False, first=first if first_number is None else first_number)
    return s, fb, pcm


@pytest.mark.parametrize("level,ch,bps,n", [
    (0, 2, 16, 1152), (2, 2, 16, 1152), (5, 2, 16, 4096), (8, 2, 16, 4096),
    (5, 1, 16, 4096), (5, 8, 16, 1152), (2, 8, 24, 192), (5, 1, 8, 4608),
    (5, 2, 8, 192), (5, 2, 24, 4608), (8, 2, 24, 1152), (0, 1, 24, 17),
    (5, 2, 16, 16), (5, 2, 16, 17), (2, 2, 16, 17), (5, 2, 16, 192), (8, 1, 16, 192), (0, 2, 8, 16),
])
def test_round_trip_fixed_blocks(level, ch, bps, n):
    p = P(level, channels=ch, bits_per_sample=bps, variable_block_size=0, allow_vbs=0)
    roundtrip(p, n, 9, tail=(n // 2 + 1) if n > 17 else 0)


@pytest.mark.parametrize("level", [10, 12])
def test_round_trip_variable_blocks(level):
    p = P(level)
    n, nb = p.block_size, 4
    first = 5 * n
    pcm = flake_amd.synth_pcm(nb, n, p.channels, p.bits_per_sample, first_frame=level)
    si = flake_amd.HostStreaminfo(min_block_size=16, max_block_size=n, sample_rate=p.sample_rate, channels=p.channels,
                                  bits_per_sample=p.bits_per_sample)
    with flake_amd.Encoder(p, max_frames=8 * nb) as enc:
        s = vbs_packed(enc, pcm, nb, n, first)
        fb, used = flake_amd.index_frames(si, s)
        assert used == len(s) and len(fb) >= nb
        decode_ok(enc, s, fb, pcm, vb=True, first=first)
        decode_ok(enc, s, fb, pcm, vb=True, first=-1)


@pytest.mark.parametrize("nframes,first,first_number", [(1, 0, 0), (63, 0, -1), (64, (1 << 31) - 70, (1 << 31) - 70),
                                                        (65, 0, 0), (80, (1 << 31) - 70, -1), (257, 0, -1), (257, 5, 5)])
def test_round_trip_frame_counts(nframes, first, first_number):
    """The remainders of a wave-per-frame grid and of the header pass's 1024 lanes' waves.  (80 frames from 2^31 - 70
    cross into the seven-byte form of the number; K4 writes that form correctly up to 2^31 + 15 -- beyond, its lead
    byte takes bits of a shift by 36 of a 32-bit number, as the reference's does, and no decoder accepts the frame.
    Longer numbers are covered by test_long_numbers_variable_blocks.)"""
    roundtrip(P(2, variable_block_size=0), 192, nframes, first=first, first_number=first_number)


def test_round_trip_64_frames_of_4096():
    roundtrip(P(5), 4096, 64, tail=777)


def test_round_trip_every_synthetic_signal():
    """synth_pcm's eight resonators and four stereo pairings (32 consecutive frames), then silence, a full-scale
    square and white noise: the CONSTANT and VERBATIM paths of this encoder."""
    roundtrip(P(5), 1152, 32)
    n = 1152
    t = np.arange(n)
    rng = np.random.RandomState(3)
    fs = (1 << 15) - 1
    frames = [np.zeros((n, 2)), np.stack([np.where(t & 1, fs, -fs - 1), np.where(t & 1, -fs - 1, fs)], axis=1),
              rng.randint(-fs - 1, fs + 1, (n, 2)), np.full((n, 2), -fs - 1), np.stack([t * 0, (t >> 3) << 4], axis=1)]
    pcm = np.concatenate(frames).astype(np.int32)
    s, fb, _ = roundtrip(P(5), n, len(frames), pcm=pcm)
    assert fb[0] < 32 and fb[3] < 32                                # silence and DC became CONSTANT subframes
    assert fb[2] > n * 2 * 2                                        # noise at full scale: more than 16 bits a sample


def test_wrong_first_number_and_uneven_blocks():
    p = P(2, variable_block_size=0, block_size=192)
    pcm = flake_amd.synth_pcm(6, 192, 2, 16)
    with flake_amd.Encoder(p, max_frames=8) as enc:
        s, fb = packed(enc, pcm, 192, 10)
        ok, out, ns, recs, summ, err = enc.decode_frames(s, fb, 6 * 192, False, 11)
        assert not ok and list(summ) == [6, 1, 0, V.V_NUMBER] and recs[0]["bit"] == 32
        assert ns == 5 * 192 and np.array_equal(out[192:], pcm.reshape(-1, 2)[192:])
        assert "frame 0" in err and "NUMBER" in err
        # a gap in the numbers: the frame behind it is blamed
        s2 = np.concatenate([s[:fb[:2].sum()], s[fb[:3].sum():]])
        fb2 = np.concatenate([fb[:2], fb[3:]])
        ok, out, ns, recs, summ, err = enc.decode_frames(s2, fb2, 5 * 192, False, 10)
        assert not ok and list(summ) == [5, 1, 2, V.V_NUMBER]
        # a shorter block in the middle of a fixed-block stream
        t96, fbt = packed(enc, flake_amd.synth_pcm(1, 96, 2, 16), 96, 12)
        s3 = np.concatenate([s[:fb[:2].sum()], t96, s[fb[:3].sum():]])
        fb3 = np.concatenate([fb[:2], fbt, fb[3:]])
        ok, out, ns, recs, summ, err = enc.decode_frames(s3, fb3, 6 * 192, False, 10)
        assert not ok and summ[2] == 2 and summ[3] == V.V_NUMBER and recs[2]["bit"] == 16


# ---- 4. int16 output -----------------------------------------------------------------------------

@pytest.mark.parametrize("bps", [16, 8])
def test_int16_output(bps):
    n, nf = 1152, 7
    p = P(5, bits_per_sample=bps, block_size=n)
    pcm = flake_amd.synth_pcm(nf, n, 2, bps).reshape(-1, 2)
    with flake_amd.Encoder(p, max_frames=nf) as enc:
        s, fb = packed(enc, pcm, n)
        wide = decode_ok(enc, s, fb, pcm, first=0).copy()
        enc.set_pcm_format(V.PCM_S16)
        narrow = decode_ok(enc, s, fb, pcm, first=0)
        assert narrow.dtype == np.int16 and np.array_equal(narrow, wide.astype(np.int16))
        # pcm_cap counts samples, not bytes: one sample short refuses the last frame and writes nothing of it
        buf, win = guarded(nf * n - 1, 2, np.int16)
        ok, out, ns, recs, summ, err = enc.decode_frames(s, fb, nf * n - 1, False, 0, out=win)
        assert not ok and list(summ) == [nf, 1, nf - 1, V.V_NUMBER] and ns == (nf - 1) * n
        assert np.array_equal(out[:ns], wide[:ns].astype(np.int16)) and guards_intact(buf, nf * n - 1)
        enc.set_pcm_format(V.PCM_S32)
        decode_ok(enc, s, fb, pcm, first=0)


# ---- 5. the device entry -------------------------------------------------------------------------

def test_device_entry(torch):
    n, nf = 1152, 12
    p = P(5, block_size=n)
    pcm = flake_amd.synth_pcm(nf, n, 2, 16)
    dev = torch.device("cuda")
    with flake_amd.Encoder(p, max_frames=nf) as enc:
        s, fb = packed(enc, pcm, n, 3)

        def encode_dev():
            dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
            info = torch.zeros(nf * 2 * V.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            stride = enc.frame_stride(n)
            frames = torch.zeros(nf * stride, dtype=torch.uint8, device=dev)
            fby = torch.zeros(nf, dtype=torch.int32, device=dev)
            slot = flake_amd.rice_slot_bytes(p, n)
            rice = torch.zeros(nf * 2 * slot, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            enc.encode_subframes_dev(dp, nf, n, info, rice_bits=rice, slot_bytes=slot, frames=frames,
                                     frame_stride=stride, frame_bytes=fby, first_frame_number=3)
            enc.sync()
            return info.cpu().numpy(), rice.cpu().numpy(), frames.cpu().numpy(), fby.cpu().numpy()

        before = encode_dev()
        ok, host_out, ns, recs, summ, _ = enc.decode_frames(s, fb, nf * n, False, 3)
        assert ok
        st = torch.cuda.Stream()
        enc.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            ds = torch.from_numpy(s).to(dev)
            dfb = torch.from_numpy(fb).to(dev)
            G = 64
            dout = torch.full(((nf * n + 2 * G) * 2,), SENT, dtype=torch.int32, device=dev)
            dsum = torch.full((4,), 99, dtype=torch.int64, device=dev)
            dns = torch.full((1,), 99, dtype=torch.int64, device=dev)
            drec = torch.full((nf, 4), 99, dtype=torch.int32, device=dev)
            st.synchronize()
            enc.decode_frames_dev(ds, len(s), dfb, nf, dout[G * 2:], nf * n, dsum, dns, drec, False, 3)
            assert enc.last_launches() == ["k_decode_frames", "k_decode", "k_decode_final"]
            enc.sync()
        got = dout.cpu().numpy().reshape(-1, 2)
        assert np.array_equal(got[G:G + nf * n], host_out) and np.array_equal(host_out, pcm.reshape(-1, 2))
        assert np.all(got[:G] == SENT) and np.all(got[G + nf * n:] == SENT)
        assert list(dsum.cpu().numpy()) == list(summ) == [nf, 0, -1, 0] and int(dns[0]) == ns == nf * n
        assert np.array_equal(drec.cpu().numpy(), recs.view(np.int32).reshape(nf, 4))
        enc.set_stream(None)
        # the workspaces are shared without harm: the encode that follows gives the bytes it gave before
        after = encode_dev()
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        # profiling brackets K7 as it brackets the others
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        assert enc.decode_frames(s, fb, nf * n, False, 3)[0]
        assert enc.kernel_times(reset=True)["k_decode"][1] == 1


# ---- 6. status codes, not faults -----------------------------------------------------------------

@pytest.fixture(scope="module")
def good8():
    n, nf = 1152, 8
    p = P(5, block_size=n)
    pcm = flake_amd.synth_pcm(nf, n, 2, 16, first_frame=40).reshape(-1, 2)
    with flake_amd.Encoder(p, max_frames=nf) as enc:
        s, fb = packed(enc, pcm, n)
    return p, n, s, fb, pcm


def run_bad(good8, stream, fb, cap=None, exact=None):
    """Decode a corrupted copy; returns (records, summary, nsamples, out).  The frames listed in exact (default: all
    but the first failing one) must hold the right samples, and the sentinels must stand."""
    p, n, _, fb0, pcm = good8
    cap = len(fb0) * n if cap is None else cap
    with flake_amd.Encoder(p, max_frames=len(fb0)) as enc:
        buf, win = guarded(cap, 2)
        ok, out, ns, recs, summ, err = enc.decode_frames(stream, fb, cap, False, 0, out=win)
        assert not ok and summ[0] == len(fb) and summ[1] >= 1
        assert guards_intact(buf, cap)
        bad = int(summ[2])
        assert recs[bad]["status"] == summ[3] != 0 and np.all(recs[:bad]["status"] == 0)
        assert f"frame {bad}," in err and V.VERIFY_STATUS[int(summ[3])] in err
        fail = enc.last_verify_failure()
        assert fail is not None and list(fail[0]) == list(summ) and fail[1]["status"] == summ[3]
        for f in (exact if exact is not None else [f for f in range(len(fb0)) if f != bad]):
            assert np.array_equal(out[f * n:(f + 1) * n], pcm[f * n:(f + 1) * n]), f
    return recs, summ, ns, out


def frame_at(fb, f):
    return int(np.sum(fb[:f]))


def test_flipped_residual_bit(good8):
    p, n, s, fb, pcm = good8
    bad = s.copy()
    bad[frame_at(fb, 3) + fb[3] // 2] ^= 0x04
    recs, summ, ns, _ = run_bad(good8, bad, fb)
    assert summ[1] == 1 and summ[2] == 3 and summ[3] in (V.V_CRC16, V.V_SYNTAX)
    assert ns == 8 * n                                            # its header was good: the range counts, unspecified


def test_flipped_header_bit(good8):
    p, n, s, fb, pcm = good8
    bad = s.copy()
    bad[frame_at(fb, 4) + 5] ^= 0x20                               # in the CRC-8 itself
    recs, summ, ns, out = run_bad(good8, bad, fb, exact=[0, 1, 2, 3])
    assert list(summ[1:]) == [1, 4, V.V_CRC8] and ns == 7 * n
    # a header that fails carries no size: the frames behind it follow the last good one, and are exact there
    assert np.array_equal(out[4 * n:7 * n], pcm[5 * n:])
    bad = s.copy()
    bad[frame_at(fb, 4) + 3] ^= 0x80                               # the channel assignment: no such stream
    recs, summ, ns, out = run_bad(good8, bad, fb, exact=[0, 1, 2, 3])
    assert list(summ[1:3]) == [1, 4] and summ[3] in (V.V_HEADER, V.V_CRC8) and ns == 7 * n
    assert np.array_equal(out[4 * n:7 * n], pcm[5 * n:])


def test_frame_size_one_too_small(good8):
    p, n, s, fb, pcm = good8
    fb2 = fb.copy()
    fb2[5] -= 1
    fb2[6] += 1                                                    # (the sizes still add up: frame 6 starts a byte early)
    recs, summ, ns, _ = run_bad(good8, s, fb2, exact=[0, 1, 2, 3, 4])
    assert summ[2] == 5 and summ[3] in (V.V_LENGTH, V.V_SYNTAX, V.V_CRC16)
    assert recs[6]["status"] == V.V_HEADER and recs[7]["status"] == 0


def test_changed_number_with_crcs_remade(good8):
    p, n, s, fb, pcm = good8
    bad = s.copy()
    a, b = frame_at(fb, 2), frame_at(fb, 3)
    assert bad[a + 4] == 2
    bad[a + 4] = 9
    bad[a + 5] = flacgen.crc8(bytes(bad[a:a + 5]))
    c16 = flacgen.crc16(bytes(bad[a:b - 2]))
    bad[b - 2], bad[b - 1] = c16 >> 8, c16 & 0xFF
    recs, summ, ns, _ = run_bad(good8, bad, fb, exact=[0, 1, 4, 5, 6, 7])
    # frame 2 does not follow frame 1, and frame 3 does not follow frame 2's 9
    assert list(summ[1:]) == [2, 2, V.V_NUMBER] and recs[3]["status"] == V.V_NUMBER and ns == 6 * n


def test_unary_run_to_the_frames_end(good8):
    p, n, s, fb, pcm = good8
    bad = s.copy()
    a, b = frame_at(fb, 6), frame_at(fb, 7)
    bad[a + fb[6] // 2:b] = 0
    recs, summ, ns, _ = run_bad(good8, bad, fb)
    assert list(summ[1:]) == [1, 6, V.V_SYNTAX] and recs[6]["bit"] == fb[6] * 8


def test_pcm_cap_one_sample_short(good8):
    p, n, s, fb, pcm = good8
    recs, summ, ns, out = run_bad(good8, s, fb, cap=8 * n - 1, exact=range(7))
    assert list(summ[1:]) == [1, 7, V.V_NUMBER] and recs[7]["bit"] == 16 and ns == 7 * n
    assert np.all(out[7 * n:] == SENT)                             # nothing of the refused frame was written


# ---- 7. refusals with nothing queued ---------------------------------------------------------------

def test_refusals(good8):
    p, n, s, fb, pcm = good8
    nf = len(fb)
    with flake_amd.Encoder(p, max_frames=nf) as enc:
        decode_ok(enc, s, fb, pcm, first=0)
        assert enc.last_launches()
        buf, win = guarded(nf * n, 2)
        recs = np.zeros(nf, V.VERIFY_REC_DTYPE)
        summ = np.full(4, 77, np.int64)
        ns = np.full(1, 77, np.int64)
        fb32 = np.ascontiguousarray(fb, np.int32)

        def call(di, do, entry="fhip_decode_frames"):
            rc = getattr(enc.lib, entry)(enc._h, di, do)
            assert rc == V.E_INVALID, rc
            assert enc.last_launches() == []
            assert guards_intact(buf, nf * n) and np.all(win == SENT) and np.all(summ == 77) and ns[0] == 77

        def din(**kw):
            d = dict(stream=s.ctypes.data, stream_bytes=len(s), frame_bytes=fb32.ctypes.data, nframes=nf,
                     variable_blocks=0, first_number=0)
            d.update(kw)
            return C.byref(V.DecodeIn(**d))

        def dout(**kw):
            d = dict(pcm=win.ctypes.data, pcm_cap=nf * n, frames=recs.ctypes.data, summary=summ.ctypes.data,
                     nsamples=ns.ctypes.data)
            d.update(kw)
            return C.byref(V.DecodeOut(**d))

        for entry in ("fhip_decode_frames", "fhip_decode_frames_dev"):
            call(None, dout(), entry)
            call(din(), None, entry)
            call(din(stream=None), dout(), entry)
            call(din(frame_bytes=None), dout(), entry)
            call(din(), dout(pcm=None), entry)
            call(din(), dout(summary=None), entry)
            call(din(), dout(nsamples=None), entry)
            call(din(nframes=nf + 1), dout(), entry)
            call(din(nframes=-1), dout(), entry)
            call(din(stream_bytes=-1), dout(), entry)
            call(din(), dout(pcm_cap=-1), entry)
            call(din(variable_blocks=2), dout(), entry)
            call(din(first_number=-2), dout(), entry)
        call(din(stream_bytes=len(s) - 1), dout())                 # the sizes do not add up (the host form knows them)
        fbx = fb32.copy()
        fbx[2] += 3
        call(din(frame_bytes=fbx.ctypes.data), dout())
        assert enc.lib.fhip_decode_frames(None, din(), dout()) == V.E_INVALID
        decode_ok(enc, s, fb, pcm, first=0)                        # the handle is as good as before
