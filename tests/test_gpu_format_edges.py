"""K5 (the verifier) and K7 (the decoder) at their internal limits: flacgen.edge_catalogue()'s frames -- partition
orders above 8 (K5 walks partitions in groups of 256), blocks on both sides of K5's residency limit, frames on both
sides of the two staging limits, block sizes around K7's 64-sample hand-over and 128-sample ring, full scale at every
sample width, LPC sums far beyond 32 bits.

The expected samples are the generator's input, which test_format_edges_cpu.py ties to the test decoder
(oracle/flac_decode.c) and whose built-for properties it reads back from the frames' bytes; nothing here is compared
with anything K5 or K7 produced.  Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
import flacgen
from flacgen import K5_MAX_PARTS, K5_RES_CAP
from test_gpu_decode import decode_ok, guarded, guards_intact

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
V = flake_amd
WINDOWS = [(0, 1), (-1, 1), (63, 2), (64, 64), (0, -1)]          # (skip, take); skip -1 stands for n - 1


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def by_handle(group):
    """The group's cases per handle: channels, width, rate, block size max(n, 16) and numbering."""
    keys = {}
    for e in flacgen.edge_cases():
        if e.group == group:
            keys.setdefault((e.channels, e.bps, e.rate, max(max(e.blocks), 16), e.vbs), []).append(e)
    assert keys
    return keys


def handles(group, max_frames=4):
    for (nch, bps, rate, bs, vbs), cases in by_handle(group).items():
        p = P(5, channels=nch, bits_per_sample=bps, sample_rate=rate, block_size=bs, allow_vbs=int(vbs))
        with flake_amd.Encoder(p, max_frames=max_frames) as enc:
            yield enc, cases


def stream_of(e):
    return np.frombuffer(e.frame, np.uint8), np.array(e.frame_bytes, np.int32)


# ---- K7 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", list("abcdef"))
def test_k7_decodes_to_the_input(group):
    count = 0
    for enc, cases in handles(group):
        for e in cases:
            s, fb = stream_of(e)
            try:
                decode_ok(enc, s, fb, e.pcm, vb=e.vbs, first=0)
                if e.bps <= 16:
                    enc.set_pcm_format(V.PCM_S16)
                    out = decode_ok(enc, s, fb, e.pcm, vb=e.vbs, first=0)
                    assert out.dtype == np.int16
                    enc.set_pcm_format(V.PCM_S32)
            except AssertionError as err:
                raise AssertionError(f"{e}: {err}") from err
            count += 1
    assert count == sum(1 for e in flacgen.edge_cases() if e.group == group)


@pytest.mark.parametrize("group", list("acd"))
def test_k7_segments_and_windows(group):
    k = len(WINDOWS)
    for enc, cases in handles(group, max_frames=3 * k + 1):
        for e in cases:
            s, fb = stream_of(e)
            n, nf = e.n, len(fb)
            for fmt in ([V.PCM_S32, V.PCM_S16] if e.bps <= 16 else [V.PCM_S32]):
                enc.set_pcm_format(fmt)
                want = e.pcm.astype(enc.pcm_dtype)
                # one segment: the whole stream
                buf, win = guarded(n, e.channels, enc.pcm_dtype)
                rc, out, ns, recs, summ, start, samples, failed, err = enc.decode_frames_segments(
                    s, fb, n, [0, nf], [0], [int(e.vbs)], out=win)
                assert rc == V.OK, (e, err)
                assert ns == n and list(summ) == [nf, 0, -1, 0] and np.all(recs["status"] == 0), e
                assert list(start) == [0] and list(samples) == [n] and list(failed) == [-1], e
                assert np.array_equal(out[:n], want) and guards_intact(buf, n), e
                # a segment per window, each the whole stream
                wins = [(n - 1 if sk < 0 else sk, tk) for sk, tk in WINDOWS]
                parts = [want[sk:n if tk < 0 else min(n, sk + tk)] for sk, tk in wins]
                total = sum(len(q) for q in parts)
                buf, win = guarded(total, e.channels, enc.pcm_dtype)
                rc, out, ns, recs, summ, start, samples, failed, err = enc.decode_frames_windows(
                    np.tile(s, k), np.tile(fb, k), total, np.arange(k + 1) * nf, [w[0] for w in wins], [w[1] for w in wins],
                    np.zeros(k, np.int64), np.full(k, int(e.vbs), np.int32), out=win)
                assert rc == V.OK, (e, err)
                assert ns == total and list(summ) == [nf * k, 0, -1, 0] and np.all(recs["status"] == 0), e
                assert list(samples) == [len(q) for q in parts] and list(failed) == [-1] * k, e
                assert list(start) == list(np.cumsum([0] + [len(q) for q in parts[:-1]])), e
                assert np.array_equal(out[:total], np.concatenate(parts)) and guards_intact(buf, total), e
            enc.set_pcm_format(V.PCM_S32)


# ---- K5 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", list("abcdef"))
def test_k5_passes_every_case(group):
    for enc, cases in handles(group):
        for e in cases:
            s, fb = stream_of(e)
            ok, recs, summ, err = enc.verify_frames(s, fb, e.pcm, 0)
            assert ok, (e, err, recs[recs["status"] != 0][:2])
            assert list(summ) == [len(fb), 0, -1, 0] and np.all(recs["status"] == 0) and np.all(recs["bit"] == -1), e
            if e.bps <= 16:                                           # the same PCM handed over as int16
                enc.set_pcm_format(V.PCM_S16)
                ok, recs, summ, err = enc.verify_frames(s, fb, e.pcm, 0)
                enc.set_pcm_format(V.PCM_S32)
                assert ok and list(summ) == [len(fb), 0, -1, 0], (e, "int16", err, recs[recs["status"] != 0][:2])


def places(e):
    """The samples to change: one of partition group 0, the first of partition 256, one of the last partition and,
    in a block that is not resident, one past the resident range."""
    n = e.n
    if e.group == "a":
        psz = e.prop["psz"]
        out = {"group 0": 3 * psz, "last partition": n - 1}
        if n > K5_MAX_PARTS * psz:
            out["partition 256"] = K5_MAX_PARTS * psz
    else:
        out = {"group 0": 100, "last partition": n - 1}
    if n > K5_RES_CAP:
        out["above the resident range"] = min(K5_RES_CAP + 12, n - 1)
    return out


@pytest.mark.parametrize("group", list("ab"))
def test_k5_reports_the_changed_sample(group):
    for enc, cases in handles(group):
        for e in cases:
            s, fb = stream_of(e)
            order = e.subs[0].get("order", 0)
            offs = e.offsets[0]
            assert len(offs) == e.n - order + 1                       # subframe 0 is FIXED or LPC in every case of a and b
            for what, i in places(e).items():
                assert order <= i < e.n
                bad = e.pcm.copy()
                bad[i, 0] += 2                                        # (any stereo transform's first subframe changes with it)
                ok, recs, summ, err = enc.verify_frames(s, fb, bad, 0)
                r = recs[0]
                assert not ok and list(summ) == [1, 1, 0, V.V_SAMPLES], (e, what, r, err)
                assert r["status"] == V.V_SAMPLES and r["sample"] == i and r["subframe"] == 0, (e, what, i, r)
                lo, hi = offs[i - order], offs[i - order + 1]
                assert lo <= r["bit"] < max(hi, lo + 1), (e, what, i, r, lo, hi)
