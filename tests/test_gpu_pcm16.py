"""int16 PCM through every layer (fhip_set_pcm_format, flake_amd_encode_frames_s16).

Every case builds int16 PCM and its int32 widening, runs both through handles that differ only in the
format, and requires byte equality of everything the entry returns.  The int32 run is the yardstick: it
is the path the rest of the suite holds to the oracle and to the reference.  Where a second witness is
cheap it is used too: the packed streams are decoded by the spec decoder of oracle/flac_decode.c and must
give back the int16 input, and the stream MD5 of a 16-bit stream must be hashlib's over the int16 bytes."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import flake_amd
from cases import _rng

pytestmark = pytest.mark.gpu

V = flake_amd
P = flake_amd.level_params

CHANNELS = (1, 2, 3, 8)
BPS = (8, 12, 16)
BLOCKS = (16, 256, 576, 1000, 1152, 4096, 4608, 8192, 16384, 20480)     # 20480: the streaming K0
LEVELS = (0, 2, 5, 8)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def signals(n, ch, bps, seed):
    """[frames][n][ch] int16, every value within bps bits: the resonator (two frames), silence, a constant,
    full-scale alternating +max / -min, three wasted bits, full-scale white noise (two frames) and full-scale noise
    of random sign (every sample +max or -min).  Returns the frames and the indices of the noise frames.
    Uniform white noise alone does not always end in K4's verbatim fallback (measured: at 8 bits FIXED order 0 with a
    Rice parameter of 7 ties with verbatim and stays); the random-sign frame does: whatever the predictor, a residual
    of magnitude 2^(bps-1) or more costs a Rice code at least bps + 1 bits, one more than a verbatim sample (stereo:
    2 bps + 2 against 2 bps + 1 per pair).  The fallback's threshold allows 16 bytes for headers (encode.c:521-527),
    so that one bit per sample decides from 128 samples up: required for n >= 256, while the 16-sample block stays
    under the threshold (measured) and is covered by the equality alone."""
    r = _rng(seed)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    t = np.arange(n)
    fr = [f for f in flake_amd.synth_pcm(2, n, ch, bps, first_frame=seed % 97)]
    fr.append(np.zeros((n, ch), np.int32))
    fr.append(np.full((n, ch), 1234 % (hi + 1), np.int32))
    fr.append(np.repeat(np.where(t & 1, hi, lo)[:, None], ch, axis=1).astype(np.int32))
    fr.append(((r.randint(lo >> 3, (hi >> 3) + 1, (n, ch))) << 3).astype(np.int32))
    white = [len(fr), len(fr) + 1]
    fr.append(r.randint(lo, hi + 1, (n, ch)).astype(np.int32))
    fr.append(r.randint(lo, hi + 1, (n, ch)).astype(np.int32))
    white.append(len(fr))
    fr.append(np.where(r.randint(0, 2, (n, ch)) > 0, hi, lo).astype(np.int32))
    pcm = np.stack(fr)
    assert pcm.min() >= lo and pcm.max() <= hi
    return np.ascontiguousarray(pcm.astype(np.int16)), white


def run_dev(torch, p, pcm, fmt, n, stage, first=0):
    """fhip_encode_subframes_dev on device tensors; everything it returns, as numpy."""
    dev = torch.device("cuda", 0)
    nfr, ch = pcm.shape[0], p.channels
    nsub = nfr * ch
    slot = V.rice_slot_bytes(p, n)
    with V.Encoder(p, max_frames=nfr) as enc:
        enc.set_pcm_format(fmt)
        stride = enc.frame_stride(n)
        pcm_t = torch.from_numpy(pcm).to(dev)
        info = torch.zeros(nsub * V.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        bits = torch.zeros(nsub * slot, dtype=torch.uint8, device=dev)
        frames = torch.zeros(nfr * stride, dtype=torch.uint8, device=dev)
        fbytes = torch.zeros(nfr, dtype=torch.int32, device=dev)
        smp = torch.zeros(nsub * n, dtype=torch.int32, device=dev) if stage else None
        autoc = torch.zeros(nsub * V.MAX_LAGS, dtype=torch.float64, device=dev) if stage else None
        torch.cuda.synchronize()
        enc.encode_subframes_dev(pcm_t, nfr, n, info, rice_bits=bits, slot_bytes=slot, samples=smp, autoc=autoc,
                                 frames=frames, frame_stride=stride, frame_bytes=fbytes, first_frame_number=first)
        enc.sync()
        out = {"launches": enc.last_launches(),
               "info_raw": info.cpu().numpy().reshape(nsub, -1).copy(),
               "bits": bits.cpu().numpy().reshape(nsub, slot).copy(),
               "frames": frames.cpu().numpy().reshape(nfr, stride).copy(),
               "frame_bytes": fbytes.cpu().numpy().copy()}
        out["info"] = np.frombuffer(out["info_raw"].tobytes(), V.INFO_DTYPE)
        if stage:
            out["samples"] = smp.cpu().numpy().copy()
            out["autoc"] = autoc.cpu().numpy().view(np.uint64).copy()      # bit patterns
    return out


def upto(a, lengths):
    """a [rows][width] with everything at or past lengths[row] zeroed."""
    return np.where(np.arange(a.shape[1])[None, :] < np.asarray(lengths)[:, None], a, 0)


def same_outputs(a, b, what):
    assert np.array_equal(a["info_raw"], b["info_raw"]), (what, "info", np.nonzero((a["info_raw"] != b["info_raw"]).any(1))[0][:4])
    if not np.array_equal(a["bits"], b["bits"]):            # (whole slots equal: the common case, and the cheap check)
        nbytes = (np.maximum(a["info"]["rice_nbits"], 0) + 7) // 8
        assert np.array_equal(upto(a["bits"], nbytes), upto(b["bits"], nbytes)), (what, "rice_bits")
    assert np.array_equal(a["frame_bytes"], b["frame_bytes"]), (what, "frame_bytes", a["frame_bytes"], b["frame_bytes"])
    assert (a["frame_bytes"] > 0).all(), (what, a["frame_bytes"])
    if not np.array_equal(a["frames"], b["frames"]):
        assert np.array_equal(upto(a["frames"], a["frame_bytes"]), upto(b["frames"], b["frame_bytes"])), (what, "frames")
    for k in ("samples", "autoc"):
        if k in a:
            assert np.array_equal(a[k], b[k]), (what, k)


def first_subframe_type(frame):
    """Type code of a frame's first subframe (frame numbers below 128, a sample rate with a code of its own)."""
    bs = frame[2] >> 4
    hdr = 4 + 1 + (1 if bs == 6 else 2 if bs == 7 else 0) + 1
    return (int(frame[hdr]) >> 1) & 0x3F


def k0_of(launches):
    return [e for e in launches if e.startswith("k_prepare")]


def device_case(torch, ch, bps, n, level, stereo=None, seed=0):
    over = {} if stereo is None else {"stereo_method": stereo}
    p = P(level, channels=ch, bits_per_sample=bps, block_size=n, variable_block_size=0, allow_vbs=0, **over)
    what = f"ch{ch} bps{bps} n{n} level{level} stereo{p.stereo_method}"
    pcm16, white = signals(n, ch, bps, seed)
    stage = level in (0, 8)            # these ask for the stage outputs (int32 rows); the others may take 16-bit rows
    a = run_dev(torch, p, pcm16, V.PCM_S16, n, stage)
    b = run_dev(torch, p, pcm16.astype(np.int32), V.PCM_S32, n, stage)
    same_outputs(a, b, what)
    k16, k32 = k0_of(a["launches"]), k0_of(b["launches"])
    assert len(k16) == 1 and "_s16" in k16[0], (what, a["launches"])
    assert len(k32) == 1 and "_s16" not in k32[0], (what, b["launches"])
    # the white-noise frames took K4's verbatim path (which reads the PCM), else the case proves nothing about it
    types = [first_subframe_type(a["frames"][f]) for f in white]
    if n >= 256:
        assert types[-1] == V.SUB_VERBATIM, (what, "no verbatim frame", types)
    return a


@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("ch", CHANNELS)
def test_device_entry_matrix(torch, ch, bps):
    """channels x bits x block sizes x levels, all six signals in every batch; for stereo also the two stereo methods
    crossed with the levels that do not have them (level 0 with the estimate, level 5 independent)."""
    count = 0
    for n in BLOCKS:
        for level in LEVELS:
            device_case(torch, ch, bps, n, level, seed=count)
            count += 1
        if ch == 2:
            device_case(torch, ch, bps, n, 0, stereo=V.STEREO_ESTIMATE, seed=count)
            device_case(torch, ch, bps, n, 5, stereo=V.STEREO_INDEPENDENT, seed=count + 1)
            count += 2
    print(f"ch{ch} bps{bps}: {count} cases identical")


def test_device_entry_benchmark_size(torch):
    """4096 x 4096 stereo, 16-bit, level 5 / LPC-8 (the headline's configuration), int16 against int32."""
    p = P(5, order_method=V.OM_MAX)
    n, nfr = 4096, 4096
    pcm = flake_amd.synth_pcm(nfr, n, 2, 16)
    a = run_dev(torch, p, np.ascontiguousarray(pcm.astype(np.int16)), V.PCM_S16, n, False)
    b = run_dev(torch, p, pcm, V.PCM_S32, n, False)
    same_outputs(a, b, "benchmark size")
    assert k0_of(a["launches"]) == ["k_prepare_stereo_s16<4,4> narrow"], a["launches"]
    assert k0_of(b["launches"]) == ["k_prepare_stereo<4,4,true> narrow"], b["launches"]
    assert a["launches"][1:] == b["launches"][1:]


def test_path_proof_and_return_to_int32(torch):
    p = P(5)
    n, nfr = 4096, 64
    pcm = flake_amd.synth_pcm(nfr, n, 2, 16)
    pcm16 = np.ascontiguousarray(pcm.astype(np.int16))
    dev = torch.device("cuda", 0)
    slot = V.rice_slot_bytes(p, n)

    def once(enc, arr):
        t = torch.from_numpy(arr).to(dev)
        info = torch.zeros(nfr * 2 * V.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        bits = torch.zeros(nfr * 2 * slot, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        enc.encode_subframes_dev(t, nfr, n, info, rice_bits=bits, slot_bytes=slot)
        enc.sync()
        return enc.last_launches(), info.cpu().numpy(), bits.cpu().numpy()

    with V.Encoder(p, max_frames=nfr) as never, V.Encoder(p, max_frames=nfr) as enc:
        ref = once(never, pcm)
        enc.set_pcm_format(V.PCM_S16)
        got16 = once(enc, pcm16)
        k16 = [e for e in got16[0] if "_s16" in e]
        assert len(k16) == 1 and k16[0].startswith("k_prepare_stereo_s16<4,4>"), got16[0]
        assert k0_of(ref[0])[0].startswith("k_prepare_stereo<4,4,true>") and got16[0][1:] == ref[0][1:]
        assert np.array_equal(got16[1], ref[1]) and np.array_equal(got16[2], ref[2])
        enc.set_pcm_format(V.PCM_S32)
        back = once(enc, pcm)
        assert back[0] == ref[0], (back[0], ref[0])
        assert not any("_s16" in e for e in back[0])
        assert np.array_equal(back[1], ref[1]) and np.array_equal(back[2], ref[2])


def batch_of(pcm, n, ch, fb, first=0):
    b = V.Batch()
    b.pcm, b.nframes, b.block_size = pcm.ctypes.data, pcm.size // (n * ch), n
    b.frame_bytes, b.first_frame_number = fb.ctypes.data, first
    return b


def packed(enc, pcm, n, first=0, steps=False):
    """fhip_encode_frames_packed, or its steps _upload + _begin + _fetch_async + _fetch_wait."""
    ch = enc.params.channels
    nf = pcm.size // (n * ch)
    fb = np.zeros(nf, np.int32)
    b = batch_of(pcm, n, ch, fb, first)
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = C.c_int64(0)
    lib, h = enc.lib, enc._h
    if not steps:
        rc = lib.fhip_encode_frames_packed(h, C.byref(b), out.ctypes.data, cap, C.byref(wrote))
    else:
        lib.fhip_frames_packed_upload.argtypes = [C.c_void_p, C.POINTER(V.Batch)]
        lib.fhip_frames_packed_fetch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.fhip_frames_packed_fetch_wait.argtypes = [C.c_void_p]
        rc = lib.fhip_frames_packed_upload(h, C.byref(b))
        if rc == 0:
            rc = lib.fhip_frames_packed_begin(h, C.byref(b), C.byref(wrote))
        if rc == 0:
            rc = lib.fhip_frames_packed_fetch_async(h, out.ctypes.data, cap)
        if rc == 0:
            rc = lib.fhip_frames_packed_fetch_wait(h)
    return rc, out[:wrote.value].copy(), fb


@pytest.mark.parametrize("ch,bps,n,level", [(2, 16, 4096, 5), (2, 16, 1152, 2), (1, 16, 4096, 5), (2, 12, 4608, 8),
                                            (8, 8, 1000, 5), (3, 16, 256, 0), (2, 16, 20480, 5)])
def test_packed_host_entries(decoder, ch, bps, n, level):
    p = P(level, channels=ch, bits_per_sample=bps, block_size=n, variable_block_size=0, allow_vbs=0)
    pcm16, white = signals(n, ch, bps, 5)
    pcm16 = np.ascontiguousarray(np.concatenate([pcm16] * 3))           # 27 frames
    pcm32 = pcm16.astype(np.int32)
    with V.Encoder(p, max_frames=len(pcm16)) as e32, V.Encoder(p, max_frames=len(pcm16)) as e16:
        e16.set_pcm_format(V.PCM_S16)
        rc, s32, fb32 = packed(e32, pcm32, n, first=3)
        assert rc == 0
        for steps in (False, True):
            rc, s16, fb16 = packed(e16, pcm16, n, first=3, steps=steps)
            assert rc == 0, e16.lib.fhip_last_error(e16._h)
            assert np.array_equal(fb16, fb32) and np.array_equal(s16, s32), (steps, fb16[:4], fb32[:4])
            assert any("_s16" in e for e in e16.last_launches())
    # an independent witness: the stream decodes to the int16 input
    out, sizes = decoder.decode(s16, ch, bps, len(pcm16) * n)
    assert len(sizes) == len(pcm16) and (np.asarray(sizes) == n).all()        # (the decoder reports block sizes)
    assert np.array_equal(out.reshape(pcm16.shape), pcm16)


@pytest.mark.parametrize("level,bps,ch", [(5, 16, 2), (8, 16, 2), (2, 12, 2), (5, 16, 6), (5, 8, 1)])
def test_prepare_ahead_changes_nothing(torch, level, bps, ch):
    p = P(level, channels=ch, bits_per_sample=bps, variable_block_size=0, allow_vbs=0)
    n, nfr = p.block_size, 70
    dev = torch.device("cuda", 0)
    slot = V.rice_slot_bytes(p, n)
    a = torch.from_numpy(flake_amd.synth_pcm(nfr, n, ch, bps, first_frame=0).astype(np.int16)).to(dev)
    b = torch.from_numpy(flake_amd.synth_pcm(nfr, n, ch, bps, first_frame=1000).astype(np.int16)).to(dev)

    def run(enc, t, hint=None):
        info = torch.zeros(nfr * ch * V.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        bits = torch.zeros(nfr * ch * slot, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        if hint is not None:
            enc.prepare_ahead(hint, nfr, n)
            assert all("_s16" in e for e in enc.last_launches()) and enc.last_launches()
        enc.encode_subframes_dev(t, nfr, n, info, rice_bits=bits, slot_bytes=slot)
        enc.sync()
        return info.cpu().numpy(), bits.cpu().numpy()

    with V.Encoder(p, max_frames=nfr) as enc:
        enc.set_pcm_format(V.PCM_S16)
        ref_a, ref_b = run(enc, a), run(enc, b)
        assert not np.array_equal(ref_a[1], ref_b[1])
        for name, t, hint, ref in (("match a", a, a, ref_a), ("match b", b, b, ref_b), ("mismatch", a, b, ref_a),
                                   ("match a again", a, a, ref_a)):
            got = run(enc, t, hint)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), name
            if hint is t:
                assert not k0_of(enc.last_launches()), (name, enc.last_launches())      # K0 ran ahead


def test_verifier_reads_int16(torch):
    p = P(5, stereo_method=V.STEREO_INDEPENDENT)          # subframe = channel
    n, nfr = 4096, 16
    pcm16 = np.ascontiguousarray(flake_amd.synth_pcm(nfr, n, 2, 16).astype(np.int16))
    pcm32 = pcm16.astype(np.int32)
    with V.Encoder(p, max_frames=nfr) as e32, V.Encoder(p, max_frames=nfr) as e16:
        e16.set_pcm_format(V.PCM_S16)
        e16.set_verify(True)
        rc, s16, fb16 = packed(e16, pcm16, n)
        assert rc == V.OK, e16.lib.fhip_last_error(e16._h)          # the run behind fhip_set_verify read int16
        rc, s32, fb32 = packed(e32, pcm32, n)
        assert rc == V.OK and np.array_equal(s16, s32) and np.array_equal(fb16, fb32)
        ok, recs, summ, err = e16.verify_frames(s16, fb16, pcm16, 0)
        assert ok and summ[0] == nfr and summ[1] == 0 and (recs["status"] == 0).all(), err
        # the device entry
        dev = torch.device("cuda", 0)
        dsum = torch.full((4,), 99, dtype=torch.int64, device=dev)
        drec = torch.zeros((nfr, 4), dtype=torch.int32, device=dev)
        e16.verify_frames_dev(torch.from_numpy(s16).to(dev), len(s16), torch.from_numpy(fb16).to(dev), nfr,
                              torch.from_numpy(pcm16.reshape(-1)).to(dev), nfr * n, 0, dsum, drec)
        e16.sync()
        assert dsum.cpu().numpy().tolist() == [nfr, 0, -1, 0]
        # one sample changed on the host: frame 3, channel 1, sample 100
        bad16 = pcm16.copy()
        bad16[3, 100, 1] += 1
        ok16, r16, sm16, err16 = e16.verify_frames(s16, fb16, bad16, 0)
        ok32, r32, sm32, err32 = e32.verify_frames(s32, fb32, bad16.astype(np.int32), 0)
        assert not ok16 and not ok32
        assert sm16.tolist() == [nfr, 1, 3, V.V_SAMPLES], (sm16, err16)
        assert (r16[3]["status"], r16[3]["subframe"], r16[3]["sample"]) == (V.V_SAMPLES, 1, 100), r16[3]
        assert np.array_equal(r16, r32) and np.array_equal(sm16, sm32) and err16 == err32


def host_stream(monkeypatch, env, level, bps, pcm, n, tail, calls):
    """calls: [(dtype, first block, blocks)] then the tail with the last call's dtype."""
    for k in ("FLAKE_AMD_BATCH", "FLAKE_AMD_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nsamp = pcm.shape[0]
    with V.HostEncoder(level=level, bits_per_sample=bps, samples=nsamp) as h:
        parts, sizes = [], []
        for i, (dt, b0, nb) in enumerate(calls):
            last = i == len(calls) - 1
            seg = pcm[b0 * n:(b0 + nb) * n + (tail if last else 0)].astype(dt)
            fn = h.encode_frames_s16 if dt == np.int16 else h.encode_frames
            s, sz = fn(seg, n, tail if last else 0)
            parts.append(s)
            sizes.append(sz)
        si = h.streaminfo()
        return np.concatenate(parts), np.concatenate(sizes), bytes(si), bytes(si.md5sum)


@pytest.mark.parametrize("env", [{"FLAKE_AMD_BATCH": "64"}, {"FLAKE_AMD_BATCH": "1024"},
                                 {"FLAKE_AMD_BATCH": "1024", "FLAKE_AMD_CHUNK": "64"}],
                         ids=["batch64", "batch1024", "batch1024_chunk64"])
def test_host_layer(monkeypatch, env):
    """300 blocks of 4096 and a tail of 1000.  FLAKE_AMD_BATCH=64 takes the single-handle route five times over;
    1024 takes it once; 1024 with FLAKE_AMD_CHUNK=64 takes the chunked two-handle route (the default chunk of 1024
    needs a batch of 2048 blocks before it chunks)."""
    n, nb, tail = 4096, 300, 1000
    pcm16 = flake_amd.synth_pcm(nb + 1, n, 2, 16).reshape(-1, 2)[:nb * n + tail].astype(np.int16)
    a = host_stream(monkeypatch, env, 5, 16, pcm16, n, tail, [(np.int16, 0, nb)])
    b = host_stream(monkeypatch, env, 5, 16, pcm16, n, tail, [(np.int32, 0, nb)])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert len(a[1]) == nb + 1
    assert a[3] == hashlib.md5(pcm16.tobytes()).digest()                # an independent MD5
    # calls of the two widths mixed on one stream
    calls = [(np.int16, 0, 75), (np.int32, 75, 75), (np.int16, 150, 75), (np.int32, 225, 75)]
    m = host_stream(monkeypatch, env, 5, 16, pcm16, n, tail, calls)
    assert np.array_equal(m[0], b[0]) and np.array_equal(m[1], b[1]) and m[2] == b[2]
    calls = [(np.int32, 0, 100), (np.int16, 100, 200)]
    m = host_stream(monkeypatch, env, 5, 16, pcm16, n, tail, calls)
    assert np.array_equal(m[0], b[0]) and m[2] == b[2]
    # 12 bits: two bytes per sample hashed, the value's low 16 bits either way
    pcm12 = flake_amd.synth_pcm(nb + 1, n, 2, 12).reshape(-1, 2)[:nb * n + tail].astype(np.int16)
    a = host_stream(monkeypatch, env, 5, 12, pcm12, n, tail, [(np.int16, 0, nb)])
    b = host_stream(monkeypatch, env, 5, 12, pcm12, n, tail, [(np.int32, 0, nb)])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    assert a[3] != bytes(16)


def test_host_layer_8_bits_and_verify(monkeypatch):
    """One byte per sample hashed at 8 bits; flake_amd_set_verify reads the int16 samples."""
    n, nb, tail = 1152, 40, 100
    pcm8 = flake_amd.synth_pcm(nb + 1, n, 2, 8).reshape(-1, 2)[:nb * n + tail].astype(np.int16)
    a = host_stream(monkeypatch, {}, 2, 8, pcm8, n, tail, [(np.int16, 0, nb)])
    b = host_stream(monkeypatch, {}, 2, 8, pcm8, n, tail, [(np.int32, 0, nb)])
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    assert a[3] == hashlib.md5(pcm8.astype(np.int8).tobytes()).digest()
    with V.HostEncoder(level=5, samples=nb * 4096) as h:
        h.set_verify(True)
        pcm = flake_amd.synth_pcm(nb, 4096, 2, 16).astype(np.int16)
        s, _ = h.encode_frames_s16(pcm, 4096)
    with V.HostEncoder(level=5, samples=nb * 4096) as h:
        s2, _ = h.encode_frames(pcm.astype(np.int32), 4096)
    assert np.array_equal(s, s2)


def test_refusals(monkeypatch):
    with V.Encoder(P(5, bits_per_sample=24), max_frames=4) as enc:
        assert enc.lib.fhip_set_pcm_format(enc._h, V.PCM_S16) == V.E_INVALID
        assert enc.lib.fhip_set_pcm_format(enc._h, 7) == V.E_INVALID
        assert enc.lib.fhip_set_pcm_format(enc._h, V.PCM_S32) == V.OK
    with V.Encoder(P(5, bits_per_sample=12), max_frames=4) as enc:
        assert enc.lib.fhip_set_pcm_format(enc._h, 2) == V.E_INVALID
        assert enc.lib.fhip_set_pcm_format(enc._h, V.PCM_S16) == V.OK
    # variable block size under int16: refused, nothing launched
    p = P(9)
    n, nblocks = p.block_size, 8
    pcm = flake_amd.synth_pcm(nblocks, n, 2, 16)
    pcm16 = np.ascontiguousarray(pcm.astype(np.int16))
    import torch
    dev = torch.device("cuda", 0)
    with V.Encoder(p, max_frames=8 * nblocks) as enc:
        frames, sizes = enc.vbs_split(pcm, n)                      # int32: works, and leaves a launch-free call behind
        packed_t = torch.zeros(8 * nblocks * enc.frame_stride(n), dtype=torch.uint8, device=dev)
        totals = torch.zeros(4, dtype=torch.int64, device=dev)
        pcm_t = torch.from_numpy(pcm).to(dev)
        torch.cuda.synchronize()
        enc.encode_blocks_vbs_dev(pcm_t, nblocks, n, packed_t, packed_t.numel(), totals)
        enc.sync()
        assert enc.last_launches()
        enc.set_pcm_format(V.PCM_S16)
        pcm16_t = torch.from_numpy(pcm16).to(dev)
        totals.fill_(-5)
        torch.cuda.synchronize()
        o = V.VbsOut(packed_t.data_ptr(), packed_t.numel(), None, None, None, totals.data_ptr())
        rc = enc.lib.fhip_encode_blocks_vbs_dev(enc._h, pcm16_t.data_ptr(), nblocks, n, 0, C.byref(o))
        assert rc == V.E_UNSUPPORTED
        assert b"int16" in enc.lib.fhip_last_error(enc._h)
        assert enc.last_launches() == []
        enc.sync()
        assert totals.cpu().numpy().tolist() == [-5] * 4            # nothing ran
        out = np.zeros(1 << 16, np.uint8)
        bb = np.full(nblocks, -7, np.int32)
        wrote = C.c_int64(-1)
        rc = enc.lib.fhip_encode_blocks_vbs_packed(enc._h, pcm16.ctypes.data, nblocks, n, 0, out.ctypes.data, out.size,
                                                   bb.ctypes.data, None, C.byref(wrote), None, None)
        assert rc == V.E_UNSUPPORTED and b"int16" in enc.lib.fhip_last_error(enc._h)
        assert enc.last_launches() == [] and (bb == -7).all() and not out.any()
        fr = np.full(nblocks, -7, np.int32)
        sz = np.full((nblocks, 8), -7, np.int32)
        rc = enc.lib.fhip_vbs_split(enc._h, pcm16.ctypes.data, nblocks, n, fr.ctypes.data, sz.ctypes.data)
        assert rc == V.E_UNSUPPORTED and b"int16" in enc.lib.fhip_last_error(enc._h)
        assert (fr == -7).all() and (sz == -7).all()
        # and back: the int32 contract is whole again
        enc.set_pcm_format(V.PCM_S32)
        f2, s2 = enc.vbs_split(pcm, n)
        assert np.array_equal(f2, frames) and np.array_equal(s2, sizes)
    # the host layer: a variable-block-size context, more than 16 bits, a CPU comparison mode
    with V.HostEncoder(level=10) as h:
        with pytest.raises(V.FlakeHipError) as ei:
            h.encode_frames_s16(pcm16[:1], n)
        assert "variable block size" in str(ei.value)
        assert h.lib.flake_amd_last_error(C.byref(h.ctx))
        s, _ = h.encode_frames(pcm[:1], n)                          # the stream is still usable
        assert len(s) > 0
    with V.HostEncoder(level=5, bits_per_sample=24) as h:
        with pytest.raises(V.FlakeHipError) as ei:
            h.encode_frames_s16(np.zeros((4096, 2), np.int16), 4096)
        assert "bits_per_sample" in str(ei.value)
    monkeypatch.setenv("FLAKE_AMD_HOST_ASSEMBLY", "1")
    with V.HostEncoder(level=5) as h:
        with pytest.raises(V.FlakeHipError) as ei:
            h.encode_frames_s16(np.zeros((4096, 2), np.int16), 4096)
        assert "FLAKE_AMD_HOST_ASSEMBLY" in str(ei.value)


# ---- the command-line encoder ------------------------------------------------------------------------------
def write_wav(path, pcm, bps, rate=44100):
    import struct
    ch = pcm.shape[1]
    nb = (bps + 7) // 8
    if nb == 2:
        raw = pcm.astype("<i2").tobytes()
    else:                                           # 3 bytes, little-endian
        raw = pcm.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
                struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * nb, ch * nb, bps) + b"data" +
                struct.pack("<I", len(raw)) + raw)
    return raw


def run_cli(args, env_over):
    import os
    import subprocess
    cli = os.path.join(flake_amd.LIB_DIR, "flake_amd_cli")
    env = {k: v for k, v in os.environ.items() if k not in ("FLAKE_AMD_HOST_ASSEMBLY", "FLAKE_AMD_HOST_VBS")}
    env.update(env_over, FLAKE_AMD_TRACE="1")
    r = subprocess.run([cli, *args], env=env, capture_output=True, text=True, timeout=300)
    widths = sorted({ln.rsplit(", ", 1)[1] for ln in r.stderr.splitlines() if ln.startswith("flake_amd batch")})
    return r, widths


def test_cli_chooses_the_entry(tmp_path, decoder):
    """A 16-bit WAV (or --synth at --bps <= 16) at a level without variable block size goes in as int16; 24 bits,
    levels 9-12 and the two CPU comparison modes keep the int32 entry and work as before, with the same bytes."""
    n_total = 4096 * 9 + 700
    pcm = flake_amd.synth_pcm(10, 4096, 2, 16).reshape(-1, 2)[:n_total]
    raw = write_wav(tmp_path / "in16.wav", pcm, 16)
    outs = {}
    for name, opts, env, want in (("default", ["-5"], {}, ["int16 samples"]),
                                  ("host_assembly", ["-5"], {"FLAKE_AMD_HOST_ASSEMBLY": "1"}, ["int32 samples"]),
                                  ("host_vbs", ["-5"], {"FLAKE_AMD_HOST_VBS": "1"}, ["int32 samples"]),
                                  ("verify", ["-5", "--verify"], {}, ["int16 samples"]),
                                  ("level10", ["-10"], {}, ["int32 samples"])):
        out = tmp_path / f"{name}.flac"
        r, widths = run_cli([*opts, str(tmp_path / "in16.wav"), str(out)], env)
        assert r.returncode == 0, (name, r.stderr)
        assert widths == want, (name, r.stderr)
        outs[name] = np.fromfile(out, dtype=np.uint8)
    for name in ("host_assembly", "host_vbs", "verify"):
        assert np.array_equal(outs[name], outs["default"]), name
    data = outs["default"]
    assert data[26:42].tobytes() == hashlib.md5(raw).digest()              # STREAMINFO's MD5 (4 + 4 + 18)
    pos = 4 + 4 + 34
    last = 0
    while not last:
        last = data[pos] >> 7
        pos += 4 + ((int(data[pos + 1]) << 16) | (int(data[pos + 2]) << 8) | int(data[pos + 3]))
    dec, sizes = decoder.decode(data[pos:], 2, 16, n_total)
    assert (dec == pcm).all() and sizes[-1] == 700
    # 24 bits: int32, as before
    pcm24 = flake_amd.synth_pcm(3, 4096, 2, 24).reshape(-1, 2)
    write_wav(tmp_path / "in24.wav", pcm24, 24)
    r, widths = run_cli(["-5", str(tmp_path / "in24.wav"), str(tmp_path / "o24.flac")], {})
    assert r.returncode == 0 and widths == ["int32 samples"], r.stderr
    # --synth
    for bps, want in ((16, "int16 samples"), (12, "int16 samples"), (24, "int32 samples")):
        r, widths = run_cli(["-5", "--synth", "20", "--bps", str(bps), str(tmp_path / f"s{bps}.flac")], {})
        assert r.returncode == 0 and widths == [want], (bps, r.stderr)


def test_overlap_split_steps_in_int16_subprocess():
    """FHIP_OVERLAP=1 (read once per process: a child) cuts a batch of >= 512 frames into two halves; the second
    half's PCM starts nframes / 2 * n * channels SAMPLES of the handle's width into the batch.  1024 frames, int16
    against int32, both split."""
    import json
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r)
        import numpy as np, flake_amd as V
        p = V.level_params(5)
        n, nfr = p.block_size, 1024
        pcm = V.synth_pcm(nfr, n, 2, 16)
        pcm[nfr // 2:] = pcm[nfr // 2:] // 3 + 5            # the halves differ
        res = []
        for fmt, arr in ((V.PCM_S32, pcm), (V.PCM_S16, pcm.astype(np.int16))):
            with V.Encoder(p, max_frames=nfr) as enc:
                enc.set_pcm_format(fmt)
                got = enc.encode_subframes(arr, n, want_residual=False, want_frames=True)
                res.append((got, enc.last_launches()))
        (a, la), (b, lb) = res
        assert a["info"].tobytes() == b["info"].tobytes()
        assert np.array_equal(a["rice_bits"], b["rice_bits"]) and np.array_equal(a["frames"], b["frames"])
        assert np.array_equal(a["frame_bytes"], b["frame_bytes"]) and (a["frame_bytes"] > 0).all()
        print("LOG " + json.dumps([la, lb]))
        print("overlap ok")
    """ % root)
    env = dict(os.environ, FHIP_OVERLAP="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overlap ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    la, lb = json.loads([x for x in r.stdout.splitlines() if x.startswith("LOG ")][0][4:])
    assert len(k0_of(la)) == 2 and len(k0_of(lb)) == 2, (la, lb)             # two halves each
    assert all("_s16" in e for e in k0_of(lb)) and not any("_s16" in e for e in k0_of(la))
