"""K7's window mode (fhip_decode_frames_windows): of every segment of a batch only samples [skip, skip + take) are
delivered, the windows back to back in pcm.

The expected samples are never the code under test's: they are slices of what the test decoder (oracle/flac_decode.c)
returns for the whole stream, cross-checked once per stream against the unchanged fhip_decode_frames.  Streams come from
tests/flacgen.py (every subframe type, wasted bits, RICE2, escapes, the four stereo assignments, fixed and variable
numbering) and from the project's encoder.  Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
import flacgen
from test_gpu_decode_segments import Stream, guarded, guards_intact

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
V = flake_amd
WINDOWS = ["k_decode_frames windows", "k_decode windows", "k_decode_final", "k_decode_seg_final"]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def win_decode(enc, s, fb, cap, sf, skip, take, num=None, var=None):
    """The host entry into an output with sentinels on both sides, which must survive."""
    buf, win = guarded(cap, enc.params.channels, enc.pcm_dtype)
    res = enc.decode_frames_windows(s, fb, cap, sf, skip, take, num, var, out=win)
    assert guards_intact(buf, cap)
    return res


def cases(n, total):
    """(skip, take) per window case for a segment of `total` samples in frames of n (the last may be shorter)."""
    return [(n + 3, 5),                   # inside one frame
            (n - 2, n + 4),               # across three frames
            (2 * n, 7),                   # from a frame's first sample
            (n + 5, 2 * n - 5),           # to a frame's last sample
            (3 * n + 1, 1),               # one sample
            (0, -1),                      # the whole segment
            (5, 0),                       # take 0
            (n, -1),                      # a skip of exactly one frame
            (total + 10, 4),              # a skip beyond the segment
            (total, -1),                  # ... and one that ends exactly at it
            (0, 2 * n),                   # two whole frames
            (total - 7, 100)]             # a take past the end: cut


def expect(ref, windows):
    """The slices of ref the windows ask for, and their lengths."""
    parts = [ref[sk:len(ref) if tk < 0 else min(len(ref), sk + tk)] for sk, tk in windows]
    return np.concatenate(parts), [len(p) for p in parts]


def one_stream_many_windows(enc, frames, ref, n, first, variable, fmts=("int32",)):
    """The run `frames` as one segment per window case; every output against slices of ref."""
    wins = cases(n, len(ref))
    k = len(wins)
    s = np.frombuffer(b"".join(frames) * k, np.uint8)
    fb = np.array([len(f) for f in frames] * k, np.int32)
    sf = np.arange(k + 1, dtype=np.int32) * len(frames)
    num, var = np.full(k, first, np.int64), np.full(k, int(variable), np.int32)
    skip, take = np.array([w[0] for w in wins], np.int64), np.array([w[1] for w in wins], np.int64)
    want, counts = expect(ref, wins)
    for fmt in fmts:
        enc.set_pcm_format(V.PCM_S16 if fmt == "int16" else V.PCM_S32)
        # the witness against the unchanged entry, once
        ok, full, ns, _, _, err = enc.decode_frames(s[:int(fb[:len(frames)].sum())], fb[:len(frames)], len(ref), variable, first)
        assert ok and ns == len(ref) and np.array_equal(full, ref.astype(enc.pcm_dtype)), err
        rc, out, ns, recs, summ, start, samples, failed, err = win_decode(enc, s, fb, len(want), sf, skip, take, num, var)
        assert rc == V.OK, err
        assert enc.last_launches() == WINDOWS
        assert ns == len(want) and list(summ) == [len(fb), 0, -1, 0] and np.all(recs["status"] == 0)
        assert list(samples) == counts and list(start) == list(np.cumsum([0] + counts[:-1])) and list(failed) == [-1] * k
        assert out.dtype == enc.pcm_dtype and np.array_equal(out, want.astype(enc.pcm_dtype))
        # one sample less of room: exactly the last delivering frame is refused, nothing is written behind pcm_cap
        cap = len(want) - 1
        rc, out, ns, recs, summ, start, samples, failed, err = win_decode(enc, s, fb, cap, sf, skip, take, num, var)
        last = len(fb) - 1                                     # (the last case ends in the segment's last frame)
        assert rc == V.E_VERIFY and list(summ) == [len(fb), 1, last, V.V_NUMBER] and recs[last]["bit"] == 16
        assert list(np.flatnonzero(recs["status"])) == [last] and list(failed) == [-1] * (k - 1) + [last]
        assert ns == len(want) - 7 and list(samples) == counts[:-1] + [0]          # (the 7 samples of the last clip)
        assert np.array_equal(out[:ns], want[:ns].astype(enc.pcm_dtype))


# ---- flacgen streams: every subframe type and channel assignment ------------------------------------

def gen_specs(n, nch, k, bps):
    """Subframe specs of frame k, rotating through the forms K7 reads; with the signal's wasted bits."""
    c4, s4 = flacgen.lpc_coefs(4, 12, seed=k)
    forms = [dict(kind="verbatim"), dict(kind="fixed", order=2, porder=2), dict(kind="lpc", order=4, coefs=c4, precision=12, shift=s4),
             dict(kind="fixed", order=1, method=1, porder=1), dict(kind="fixed", order=2, porder=2, escape=(1,)),
             dict(kind="fixed", order=3, wasted=2, porder=0), dict(kind="constant"), dict(kind="fixed", order=4, porder=1)]
    return [forms[(k + c) % len(forms)] for c in range(nch)]


def gen_stream(n, nch, ch_code, bps, vbs, nframes=6, first=3, tail=0):
    """(frames, first number): nframes frames of n samples (and one of `tail`) written by flacgen."""
    frames = []
    sizes = [n] * nframes + ([tail] if tail else [])
    number = first
    for k, m in enumerate(sizes):
        specs = gen_specs(m, nch, k, bps)
        stereo = ch_code is not None and ch_code >= 8
        if stereo:                       # (the subframes are not the channels: keep to forms any values take)
            specs = [sp if sp["kind"] not in ("constant",) and not sp.get("wasted") else dict(kind="fixed", order=2, porder=1)
                     for sp in specs]
        pcm = flacgen.test_signal(m, nch, bps, seed=100 * n + 10 * k + nch)
        for c, sp in enumerate(specs):
            if stereo:
                continue
            if sp["kind"] == "constant":
                pcm[:, c] = -5 - c
            elif sp.get("wasted"):
                pcm[:, c] = (pcm[:, c] >> sp["wasted"]) << sp["wasted"]
        frames.append(flacgen.frame(pcm, number, bps, 44100, specs, ch_code=ch_code, vbs=vbs))
        number += m if vbs else 1
    return frames, first


GEN = [(16, 1, None, 16, False), (192, 1, None, 8, True), (16, 2, 1, 16, True), (192, 2, 8, 16, False), (16, 2, 9, 24, False),
       (192, 2, 10, 24, True), (16, 2, 10, 8, False), (16, 3, None, 8, True), (192, 3, None, 24, False)]


@pytest.mark.parametrize("n,nch,ch_code,bps,vbs", GEN)
def test_generated_streams(decoder, n, nch, ch_code, bps, vbs):
    frames, first = gen_stream(n, nch, ch_code, bps, vbs, tail=n - 4)
    ref, sizes = decoder.decode(np.frombuffer(b"".join(frames), np.uint8), nch, bps, 7 * n)
    assert list(sizes) == [n] * 6 + [n - 4]
    p = P(5, channels=nch, bits_per_sample=bps, block_size=n, variable_block_size=0)
    with flake_amd.Encoder(p, max_frames=7 * 12) as enc:
        one_stream_many_windows(enc, frames, ref, n, first, vbs, ("int32", "int16") if bps <= 16 else ("int32",))


# ---- the encoder's streams ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,ch,bps", [(16, 1, 16), (192, 2, 16), (192, 3, 24), (16, 2, 8)])
def test_encoded_streams(decoder, n, ch, bps):
    p = P(5, channels=ch, bits_per_sample=bps, block_size=n, variable_block_size=0)
    with flake_amd.Encoder(p, max_frames=7 * 12) as enc:
        a = Stream(enc, 6, n, 9, 21, tail=n - 4)
        ref, sizes = decoder.decode(a.s, ch, bps, len(a.pcm))
        assert np.array_equal(ref, a.pcm) and list(sizes) == a.sizes
        frames = [a.s[a.off[i]:a.off[i + 1]].tobytes() for i in range(len(a.fb))]
        one_stream_many_windows(enc, frames, ref, n, 9, False, ("int32", "int16") if bps <= 16 else ("int32",))


@pytest.fixture(scope="module")
def long_stream(decoder):
    """1100 mono frames of 16 samples numbered from 0, and the test decoder's samples of them."""
    p = P(5, channels=1, block_size=16, variable_block_size=0)
    with flake_amd.Encoder(p, max_frames=1100) as enc:
        a = Stream(enc, 1100, 16, 0, 1)
    ref, sizes = decoder.decode(a.s, 1, 16, len(a.pcm))
    assert len(sizes) == 1100 and np.array_equal(ref, a.pcm)
    ref.setflags(write=False)
    return a, ref


@pytest.mark.parametrize("form", ["forty", "single", "frames_1020_to_1030"])
@pytest.mark.parametrize("fmt", ["int32", "int16"])
def test_segments_across_the_header_pass_chunk(long_stream, form, fmt):
    """Segments straddle the header pass's chunk of 1024 frames: the segment's head lies in the chunk before."""
    a, ref = long_stream
    if form == "forty":
        rng = np.random.default_rng(5)
        cuts = np.sort(rng.choice(np.arange(1, 1100), 39, replace=False))
        cuts[np.argmin(np.abs(cuts - 1024))] = 1019                    # one segment begins at 1019 and straddles 1024
        cuts = np.unique(cuts)
        sf = np.concatenate([[0], cuts, [1100]]).astype(np.int32)
        assert not np.any(sf == 1024)
        lens = np.diff(sf) * 16
        skip = np.array([rng.integers(0, ln + 3) for ln in lens], np.int64)
        take = np.array([-1 if i % 5 == 0 else rng.integers(0, ln + 3) for i, ln in enumerate(lens)], np.int64)
        skip[np.searchsorted(sf, 1019)] = 4 * 16 + 7                      # ... and its window begins behind the boundary
    elif form == "single":
        sf, skip, take = np.array([0, 1100], np.int32), np.array([1000 * 16 + 3], np.int64), np.array([50 * 16], np.int64)
    else:
        sf, skip, take = np.array([0, 1100], np.int32), np.array([1020 * 16 + 5], np.int64), np.array([10 * 16 + 4], np.int64)
    num = sf[:-1].astype(np.int64)
    parts = [ref[16 * sf[i]:16 * sf[i + 1]] for i in range(len(sf) - 1)]
    want = [expect(part, [(int(sk), int(tk))]) for part, sk, tk in zip(parts, skip, take)]
    counts = [w[1][0] for w in want]
    want = np.concatenate([w[0] for w in want])
    with flake_amd.Encoder(P(5, channels=1, block_size=16, variable_block_size=0), max_frames=1100) as enc:
        if fmt == "int16":
            enc.set_pcm_format(V.PCM_S16)
        rc, out, ns, recs, summ, start, samples, failed, err = win_decode(enc, a.s, a.fb, len(want), sf, skip, take, num)
        assert rc == V.OK, err
        assert ns == len(want) and list(samples) == counts and list(start) == list(np.cumsum([0] + counts[:-1]))
        assert np.array_equal(out, want.astype(enc.pcm_dtype)) and list(failed) == [-1] * len(counts)
        if form == "frames_1020_to_1030":
            assert counts == [10 * 16 + 4] and np.array_equal(want, ref[1020 * 16 + 5:1030 * 16 + 9])


# ---- failures ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three(decoder):
    """Three streams of 7 frames of 64 stereo samples with different first numbers; the decoder's samples of each."""
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        st = [Stream(enc, 7, 64, first, seed) for first, seed in ((0, 1), (100, 2), (7, 3))]
    refs = [decoder.decode(x.s, 2, 16, len(x.pcm))[0] for x in st]
    for x, r in zip(st, refs):
        assert np.array_equal(r, x.pcm)
    return st, refs


@pytest.mark.parametrize("where", ["inside_the_window", "clipped_away"])
def test_a_flipped_bit_in_the_middle_window(three, where):
    st, refs = three
    s = np.concatenate([x.s for x in st])
    fb = np.concatenate([x.fb for x in st]).astype(np.int32)
    sf, num = np.array([0, 7, 14, 21], np.int32), np.array([0, 100, 7], np.int64)
    wins = [(70, 200), (3 * 64 + 10, 100), (0, 64 * 7 - 1)]            # the middle one: frames 3 and 4 of its stream
    want = [expect(r, [w])[0] for r, w in zip(refs, wins)]
    f = 7 + (3 if where == "inside_the_window" else 0)                 # frame 0 of the stream delivers nothing
    off = np.concatenate([[0], np.cumsum(fb)])
    bad = s.copy()
    bad[off[f + 1] - 3] ^= 0x04                                        # in the frame's last residuals: CRC-16 at the least
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        total = sum(len(w) for w in want)
        rc, out, ns, recs, summ, start, samples, failed, err = win_decode(enc, bad, fb, total, sf, [w[0] for w in wins],
                                                                          [w[1] for w in wins], num)
        assert rc == V.E_VERIFY
        status = int(recs[f]["status"])
        assert status != 0 and list(np.flatnonzero(recs["status"])) == [f]
        assert list(summ) == [21, 1, f, status] and list(failed) == [-1, f, -1]
        # the frame was placed and counted (its own range is unspecified); the neighbours are exact where the call says
        assert list(samples) == [len(w) for w in want] and ns == total
        assert list(start) == [0, len(want[0]), len(want[0]) + len(want[1])]
        for k in (0, 2):
            assert np.array_equal(out[start[k]:start[k] + samples[k]], want[k])
        if where == "clipped_away":                                    # the failing frame had nothing to deliver
            assert np.array_equal(out[start[1]:start[1] + samples[1]], want[1])
        else:
            keep = np.ones(100, bool)
            keep[:64 - 10] = False                                     # frame 3's share of the window
            assert np.array_equal(out[start[1]:start[1] + 100][keep], want[1][keep])


def test_a_broken_header_takes_no_room_in_its_segment(three):
    """A header that does not parse carries no size: the segment's samples behind it move up, as placement always had it."""
    st, refs = three
    x, ref = st[1], refs[1]
    bad = x.s.copy()
    bad[x.off[2] + 1] ^= 0x40                                          # the sync code of frame 2
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        rc, out, ns, recs, summ, start, samples, failed, err = win_decode(enc, bad, x.fb, 100, [0, 7], [100], [100], [100])
        assert rc == V.E_VERIFY and list(failed) == [2] and recs[2]["status"] in (V.V_HEADER, V.V_CRC8)
        # frames 0, 1, 3, ... of the stream count 64 each: samples 100 .. 200 of that sequence (frame 3 has no good
        # predecessor to be held against)
        seq = np.concatenate([ref[:128], ref[192:]])
        assert list(np.flatnonzero(recs["status"])) == [2] and list(summ) == [7, 1, 2, int(recs[2]["status"])]
        assert ns == 100 and list(samples) == [100] and list(start) == [0]
        assert np.array_equal(out, seq[100:200])


# ---- arguments and the other entries' launch lists ---------------------------------------------------

def test_bad_arguments_queue_nothing(three, torch):
    st, refs = three
    x = st[0]
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        good = enc.decode_frames_windows(x.s, x.fb, 64, [0, 7], [10], [20], [0])
        assert good[0] == V.OK and enc.last_launches() == WINDOWS and good[2] == 20
        for kw in (dict(null_table="skip"), dict(null_table="take"), dict(null_table="win"), dict(null_table="segs")):
            res = enc.decode_frames_windows(x.s, x.fb, 64, [0, 7], [10], [20], [0], **kw)
            assert res[0] == V.E_INVALID and enc.last_launches() == [], kw
            assert np.all(res[1] == 0) and np.all(res[5] == -7)          # nothing came back
        for skip, take in (([-1], [20]), ([10], [-2])):
            res = enc.decode_frames_windows(x.s, x.fb, 64, [0, 7], skip, take, [0])
            assert res[0] == V.E_INVALID and enc.last_launches() == [] and np.all(res[1] == 0)
        # the device form checks the pointers
        dev = torch.device("cuda", 0)
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)          # noqa: E731
        t32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)          # noqa: E731
        d = dict(stream=torch.from_numpy(x.s).to(dev), stream_bytes=len(x.s), frame_bytes=t32(x.fb), nframes=7,
                 pcm=torch.zeros(64 * 2, dtype=torch.int32, device=dev), pcm_cap=64, summary=t64([0] * 4), nsamples=t64([0]),
                 seg_first=t32([0, 7]), nsegs=1, seg_number=t64([0]), seg_variable=t32([0]), seg_start=t64([0]),
                 seg_samples=t64([0]), seg_failed=t32([0]), seg_skip=t64([10]), seg_take=t64([20]))
        torch.cuda.synchronize()
        for name in ("seg_skip", "seg_take"):
            assert enc.decode_frames_windows_dev(**{**d, name: None}) == V.E_INVALID and enc.last_launches() == []
        assert enc.decode_frames_windows_dev(**d) == V.OK and enc.last_launches() == WINDOWS
        enc.sync()
        assert d["nsamples"].item() == 20 and d["seg_samples"].item() == 20 and d["seg_start"].item() == 0
        assert np.array_equal(d["pcm"].cpu().numpy().reshape(64, 2)[:20], refs[0][10:30])
        assert list(d["summary"].cpu().numpy()) == [7, 0, -1, 0]


def test_the_other_entries_keep_their_launch_lists(three):
    st, refs = three
    x = st[0]
    with flake_amd.Encoder(P(5, block_size=64, variable_block_size=0), max_frames=32) as enc:
        ok, out, ns, _, _, _ = enc.decode_frames(x.s, x.fb, len(x.pcm), False, 0)
        assert ok and enc.last_launches() == ["k_decode_frames", "k_decode", "k_decode_final"]
        res = enc.decode_frames_segments(x.s, x.fb, len(x.pcm), [0, 3, 7], [0, 3])
        assert res[0] == V.OK
        assert enc.last_launches() == ["k_decode_frames segments", "k_decode", "k_decode_final", "k_decode_seg_final"]
        assert np.array_equal(res[1], out) and np.array_equal(out, refs[0])
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        assert enc.decode_frames_windows(x.s, x.fb, 64, [0, 7], [10], [20], [0])[0] == V.OK
        assert enc.kernel_times(reset=True)["k_decode"][1] == 1        # timed as "k_decode"
