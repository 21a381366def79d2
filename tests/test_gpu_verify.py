"""K5, the on-device verifier (fhip_verify_frames*, fhip_set_verify): good streams pass, broken ones fail
at the right frame, sample and status, and verification changes no output byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flake_amd
import flacgen
import oraclelib
from cases import param_sets

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
V = flake_amd


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def packed(enc, pcm, n, first=0):
    """fhip_encode_frames_packed: (rc, stream bytes, frame sizes)."""
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
    return rc, out[:wrote.value].copy(), fb


def vbs_packed(enc, pcm, nblocks, n, first=0):
    pcm = np.ascontiguousarray(pcm, np.int32)
    cap = 8 * nblocks * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    bb = np.zeros(nblocks, np.int32)
    wrote = C.c_int64(0)
    mx, nxt = C.c_int(0), C.c_uint32(0)
    rc = enc.lib.fhip_encode_blocks_vbs_packed(enc._h, pcm.ctypes.data, nblocks, n, first, out.ctypes.data, cap,
                                               bb.ctypes.data, None, C.byref(wrote), C.byref(mx), C.byref(nxt))
    return rc, out[:wrote.value].copy()


def check_ok(enc, stream, fb, pcm, first, torch=None):
    ok, recs, summ, err = enc.verify_frames(stream, fb, pcm, first)
    assert ok, (err, recs[recs["status"] != 0][:4])
    assert summ[0] == len(fb) and summ[1] == 0 and summ[2] == -1
    assert np.all(recs["status"] == 0)
    if torch is not None:
        dev = torch.device("cuda")
        ds = torch.from_numpy(np.ascontiguousarray(stream)).to(dev)
        dfb = torch.from_numpy(np.ascontiguousarray(fb)).to(dev)
        dp = torch.from_numpy(np.ascontiguousarray(pcm, np.int32).reshape(-1)).to(dev)
        dsum = torch.full((4,), 99, dtype=torch.int64, device=dev)
        drec = torch.zeros((len(fb), 4), dtype=torch.int32, device=dev)
        enc.verify_frames_dev(ds, len(stream), dfb, len(fb), dp, pcm.reshape(-1, enc.params.channels).shape[0],
                              first, dsum, drec)
        enc.sync()
        s = dsum.cpu().numpy()
        assert s[0] == len(fb) and s[1] == 0 and s[2] == -1, s
        assert int(drec[:, 0].abs().sum()) == 0


def roundtrip_fixed(p, n, nframes, torch=None, tail=0, seed=0):
    """Encode nframes (+ a ragged tail batch) with verification off and on; check K5's verdicts."""
    pcm = flake_amd.synth_pcm(nframes, n, p.channels, p.bits_per_sample, first_frame=seed)
    with flake_amd.Encoder(p, max_frames=nframes) as enc:
        rc, s0, fb0 = packed(enc, pcm, n)
        assert rc == 0
        check_ok(enc, s0, fb0, pcm, 0, torch)
        enc.set_verify(True)
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        rc, s1, fb1 = packed(enc, pcm, n)
        assert rc == 0, enc.lib.fhip_last_error(enc._h)
        assert np.array_equal(s0, s1) and np.array_equal(fb0, fb1)
        kt = enc.kernel_times(reset=True)
        assert kt["k_verify"][1] > 0
        if tail:
            tp = flake_amd.synth_pcm(1, tail, p.channels, p.bits_per_sample, first_frame=seed + 99)
            first = nframes if not p.allow_vbs else nframes * n
            rc, st, fbt = packed(enc, tp, tail, first=first)
            assert rc == 0, enc.lib.fhip_last_error(enc._h)
            # the whole stream, tail included, through the caller's entry
            full = np.concatenate([pcm.reshape(-1, p.channels), tp.reshape(-1, p.channels)])
            q = p.copy()
            q.block_size = n
            with flake_amd.Encoder(q, max_frames=4) as e2:
                check_ok(e2, np.concatenate([s0, st]), np.concatenate([fb0, fbt]), full, 0)
    return s0, fb0, pcm


@pytest.mark.parametrize("name,p,n", param_sets(), ids=[c[0] for c in param_sets()])
def test_configs_pass(torch, name, p, n):
    p = p.copy()
    p.variable_block_size = 0
    p.block_size = n
    roundtrip_fixed(p, n, 24, torch, tail=n // 3 + 1)


@pytest.mark.parametrize("level", range(13))
def test_levels_fixed_pass(torch, level):
    p = P(level, variable_block_size=0)
    roundtrip_fixed(p, p.block_size, 16, torch if level % 4 == 0 else None, tail=777)


@pytest.mark.parametrize("level", [9, 10, 11, 12])
def test_levels_vbs_pass(torch, level):
    p = P(level)
    assert p.variable_block_size
    n, nb = p.block_size, 8
    pcm = flake_amd.synth_pcm(nb, n, p.channels, p.bits_per_sample, first_frame=level)
    with flake_amd.Encoder(p, max_frames=8 * nb) as enc:
        rc, s0 = vbs_packed(enc, pcm, nb, n, first=5 * n)
        assert rc == 0
        # frame sizes from the device entry, which reports them
        dev = torch.device("cuda")
        dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
        cap = len(s0) + 4096
        dpk = torch.zeros(cap, dtype=torch.uint8, device=dev)
        dfb = torch.zeros(8 * nb, dtype=torch.int32, device=dev)
        dt = torch.zeros(4, dtype=torch.int64, device=dev)
        enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt, frame_bytes=dfb, first_frame_number=5 * n)
        enc.sync()
        t = dt.cpu().numpy()
        nf = int(t[0])
        fb = dfb.cpu().numpy()[:nf]
        assert np.array_equal(dpk.cpu().numpy()[:t[1]], s0)
        check_ok(enc, s0, fb, pcm, 5 * n, torch)
        enc.set_verify(True)
        rc, s1 = vbs_packed(enc, pcm, nb, n, first=5 * n)
        assert rc == 0, enc.lib.fhip_last_error(enc._h)
        assert np.array_equal(s0, s1)
        dt.zero_()
        enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt, first_frame_number=5 * n)
        enc.sync()
        assert int(dt[3]) & 4 == 0
        assert np.array_equal(dpk.cpu().numpy()[:len(s0)], s0)
        # the wrong PCM sets the flag (and only the flag)
        dp2 = dp.clone()
        dp2[n * 2 + 7] += 3
        dt.zero_()
        dsum = torch.zeros(4, dtype=torch.int64, device=dev)
        enc.verify_frames_dev(dpk, int(t[1]), dfb, nf, dp2, nb * n, 5 * n, dsum)
        enc.sync()
        assert int(dsum[1]) == 1


@pytest.mark.parametrize("ch,bps,n", [(1, 16, 4096), (3, 16, 4096), (8, 16, 1152), (2, 8, 4096), (2, 12, 4096),
                                      (2, 20, 4096), (2, 24, 4608), (1, 32, 1152), (2, 32, 2048), (2, 16, 16),
                                      (2, 16, 192), (2, 16, 1152), (1, 16, 4608), (2, 16, 65535),
                                      (2, 24, 16384), (2, 16, 1000)])
def test_shapes_pass(torch, ch, bps, n):
    p = P(5, channels=ch, bits_per_sample=bps, block_size=n, max_partition_order=8 if n >= 4096 else 3)
    roundtrip_fixed(p, n, 3 if n > 16384 else 8, torch, tail=(n // 2 + 1) if n > 16 else 0)


def test_flacgen_frames_pass():
    for name, pcm, fr, bps, sr, nch in flacgen.catalogue():
        p = P(5, channels=nch, bits_per_sample=bps, sample_rate=sr, block_size=max(len(pcm), 16))
        with flake_amd.Encoder(p, max_frames=2) as enc:
            ok, recs, summ, err = enc.verify_frames(np.frombuffer(fr, np.uint8), [len(fr)], pcm, 0)
            assert ok, (name, err)
    for first, pcm, fr in flacgen.utf8_catalogue():
        p = P(9, channels=1, block_size=4096)
        with flake_amd.Encoder(p, max_frames=2) as enc:
            ok, recs, summ, err = enc.verify_frames(np.frombuffer(fr, np.uint8), [len(fr)], pcm, first)
            assert ok, (first, err)


def test_flacgen_wrong_pcm_fails():
    for name, pcm, fr, bps, sr, nch in flacgen.catalogue():
        p = P(5, channels=nch, bits_per_sample=bps, sample_rate=sr, block_size=max(len(pcm), 16))
        bad = pcm.copy()
        i = len(pcm) // 2 + 3
        bad[i, 0] += 2
        with flake_amd.Encoder(p, max_frames=2) as enc:
            ok, recs, summ, err = enc.verify_frames(np.frombuffer(fr, np.uint8), [len(fr)], bad, 0)
            assert not ok, name
            assert recs[0]["status"] == V.V_SAMPLES and recs[0]["sample"] == i, (name, recs[0])


def test_oracle_encoded_frames_pass(oracle):
    """Frames the CPU oracle wrote (not the GPU encoder), through the host-pointer entry."""
    for level in (0, 2, 5, 8):
        p = P(level, variable_block_size=0)
        n = p.block_size
        pcm = flake_amd.synth_pcm(6, n, 2, 16, first_frame=3)
        frames = []
        for f in range(6):
            rc, fr, _, _, _ = oracle.encode_frame(p, f, pcm[f], n)
            assert rc > 0
            frames.append(fr)
        with flake_amd.Encoder(p, max_frames=8) as enc:
            ok, recs, summ, err = enc.verify_frames(np.concatenate(frames), [len(q) for q in frames],
                                                    pcm.reshape(-1, 2), 0)
            assert ok, (level, err)


def _stream64(seed=0):
    p = P(5)
    n = 1152
    p.block_size = n
    pcm = flake_amd.synth_pcm(64, n, 2, 16, first_frame=seed)
    with flake_amd.Encoder(p, max_frames=64) as enc:
        rc, s, fb = packed(enc, pcm, n)
    assert rc == 0
    return p, n, pcm, s, fb


def test_single_bit_flips_fail_exactly_their_frame():
    p, n, pcm, s, fb = _stream64(1)
    off = np.concatenate([[0], np.cumsum(fb)])
    rng = np.random.default_rng(123)
    with flake_amd.Encoder(p, max_frames=64) as enc:
        for _ in range(2000):
            bit = int(rng.integers(0, len(s) * 8))
            t = s.copy()
            t[bit >> 3] ^= np.uint8(0x80 >> (bit & 7))
            f = int(np.searchsorted(off, bit >> 3, side="right") - 1)
            ok, recs, summ, err = enc.verify_frames(t, fb, pcm.reshape(-1, 2), 0)
            bad = np.nonzero(recs["status"])[0]
            assert not ok and list(bad) == [f], (bit, f, bad, recs[bad][:3])
            assert summ[1] == 1 and summ[2] == f


def _header_bytes(fr):
    """Byte length of a frame header (CRC-8 included) as this encoder writes it."""
    b0 = fr[4]
    extra = 0
    if b0 >= 0x80:
        ones = 0
        while ones < 8 and (b0 << ones) & 0x80:
            ones += 1
        extra = ones - 1
    h = 5 + extra
    bs, sr = fr[2] >> 4, fr[2] & 15
    h += {6: 1, 7: 2}.get(bs, 0) + {12: 1, 13: 2, 14: 2}.get(sr, 0)
    return h + 1


def test_flips_with_crcs_recomputed_match_the_oracle_decoder():
    """Bits flipped in the subframes with CRC-16 recomputed: only decoding logic can tell.  K5 fails a frame
    exactly when the oracle decoder errors or decodes other samples -- except for the one check the oracle
    decoder does not make, the zero padding before CRC-16 (status PADDING).  Header fields (codes,
    numbering) are not flipped here: the oracle does not check them either."""
    p, n, pcm, s, fb = _stream64(2)
    off = np.concatenate([[0], np.cumsum(fb)])
    dec = oraclelib.Decoder()
    rng = np.random.default_rng(7)
    x = pcm.reshape(-1, 2)
    with flake_amd.Encoder(p, max_frames=64) as enc:
        for _ in range(600):
            f = int(rng.integers(0, 64))
            fr = bytearray(s[off[f]:off[f + 1]].tobytes())
            h = _header_bytes(fr)
            bit = int(rng.integers(h * 8, (len(fr) - 2) * 8))
            fr[bit >> 3] ^= 0x80 >> (bit & 7)
            fr[-2:] = flacgen.crc16(bytes(fr[:-2])).to_bytes(2, "big")
            want = x[f * n:(f + 1) * n]
            try:
                got, _ = dec.decode(np.frombuffer(bytes(fr), np.uint8), 2, 16, n + 65536)
                oracle_ok = got.shape == want.shape and np.array_equal(got, want)
            except ValueError:
                oracle_ok = False
            ok, recs, summ, err = enc.verify_frames(np.frombuffer(bytes(fr), np.uint8), [len(fr)], want, f * n)
            if recs[0]["status"] == V.V_PADDING:
                assert oracle_ok
                continue
            assert ok == oracle_ok, (f, bit, recs[0], err)


def test_pcm_mutations_report_the_sample():
    p, n, pcm, s, fb = _stream64(3)
    off = np.concatenate([[0], np.cumsum(fb)])
    rng = np.random.default_rng(11)
    with flake_amd.Encoder(p, max_frames=64) as enc:
        for _ in range(200):
            f, c, i = int(rng.integers(0, 64)), int(rng.integers(0, 2)), int(rng.integers(0, n))
            x = pcm.reshape(-1, 2).copy()
            l0, r0 = int(x[f * n + i, 0]), int(x[f * n + i, 1])
            x[f * n + i, c] += int(rng.choice([-5, -1, 1, 2, 1000]))
            l1, r1 = int(x[f * n + i, 0]), int(x[f * n + i, 1])
            cc = s[off[f] + 3] >> 4
            if cc < 8:
                sub = c
            elif cc == 8:
                sub = 0 if l1 != l0 else 1
            elif cc == 9:
                sub = 0
            else:
                sub = 0 if (l1 + r1) >> 1 != (l0 + r0) >> 1 else 1
            ok, recs, summ, err = enc.verify_frames(s, fb, x, 0)
            assert not ok
            assert list(np.nonzero(recs["status"])[0]) == [f]
            r = recs[f]
            assert r["status"] == V.V_SAMPLES and r["sample"] == i and r["subframe"] == sub, (f, c, i, cc, r)


def test_broken_framing_is_caught():
    p, n, pcm, s, fb = _stream64(4)
    off = np.concatenate([[0], np.cumsum(fb)])
    x = pcm.reshape(-1, 2)
    frames = [s[off[f]:off[f + 1]] for f in range(64)]
    cases = {}
    for d in (-1, 1):
        g = fb.copy()
        g[10] += d
        cases[f"size{d:+d}"] = (s, g)
    sw = frames[:]
    sw[20], sw[21] = sw[21], sw[20]
    cases["swap"] = (np.concatenate(sw), np.array([len(q) for q in sw], np.int32))
    dr = frames[:30] + frames[31:]
    cases["drop"] = (np.concatenate(dr), np.array([len(q) for q in dr], np.int32))
    du = frames[:30] + [frames[30]] + frames[30:]
    cases["dup"] = (np.concatenate(du), np.array([len(q) for q in du], np.int32))
    cases["truncated"] = (s[:off[40] + 100], fb)
    with flake_amd.Encoder(p, max_frames=80) as enc:
        for name, (st, g) in cases.items():
            ok, recs, summ, err = enc.verify_frames(st, g, x, 0)
            assert not ok, name
            assert summ[3] in (V.V_LENGTH, V.V_NUMBER), (name, summ, err)
        enc.sync()


def test_host_layer_verify_identical_bytes():
    for level in range(13):
        pcm = flake_amd.synth_pcm(40, 4096 if level > 2 else 1152, 2, 16, first_frame=level).reshape(-1, 2)
        bs = 4096 if level > 2 else 1152
        if level >= 11:
            bs = 8192
            pcm = pcm[: (len(pcm) // bs) * bs]
        outs = []
        for on in (False, True):
            with flake_amd.HostEncoder(level) as he:
                if on:
                    he.set_verify(True)
                tail = len(pcm) % bs
                data, _ = he.encode_frames(pcm, bs, tail)
                outs.append(data)
        assert np.array_equal(outs[0], outs[1]), level


def test_host_layer_chunked_and_compare_modes():
    pcm = flake_amd.synth_pcm(2200, 1152, 2, 16).reshape(-1, 2)
    base = None
    for env in ({"FLAKE_AMD_BATCH": "4096", "FLAKE_AMD_CHUNK": "512"}, {"FLAKE_AMD_HOST_ASSEMBLY": "1"},
                {"FLAKE_AMD_HOST_VBS": "1"}):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            outs = []
            for on in (False, True):
                with flake_amd.HostEncoder(2) as he:
                    he.set_verify(on)
                    data, _ = he.encode_frames(pcm, 1152)
                    outs.append(data)
            assert np.array_equal(outs[0], outs[1]), env
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v


def test_cli_verify(tmp_path):
    cli = os.path.join(os.path.dirname(flake_amd.__file__), "lib", "flake_amd_cli")
    out = tmp_path / "out.flac"
    r = subprocess.run([cli, "--verify", "--synth", "64", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.stat().st_size > 1000
