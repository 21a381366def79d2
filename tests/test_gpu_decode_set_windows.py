"""flake_amd_decode_set_windows: windows of samples out of many streams in shared device batches.  Eight streams of 40
frames of 192 stereo samples (the last frame 100) run with FLAKE_AMD_BATCH=16, so that batches are cut inside windows;
each stream gets a window asked of the whole stream, one asked of a run that starts at frame 7 and one asked of a run
that is only the short last frame.  The expected samples are slices of what the test decoder (oracle/flac_decode.c)
returns for each whole stream; every comparison is exact."""
import hashlib

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
from test_gpu_decode_segments import Stream

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
V = flake_amd
N, NF, TAIL, BATCH = 192, 40, 100, 16
TOTAL = (NF - 1) * N + TAIL


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def like(bps=16):
    return V.HostStreaminfo(min_block_size=N, max_block_size=N, sample_rate=44100, channels=2, bits_per_sample=bps)


@pytest.fixture(scope="module")
def streams(decoder):
    with flake_amd.Encoder(P(5, block_size=N, variable_block_size=0), max_frames=NF) as enc:
        st = [Stream(enc, NF - 1, N, 0, 10 + s, tail=TAIL) for s in range(8)]
    refs = []
    for x in st:
        ref, sizes = decoder.decode(x.s, 2, 16, TOTAL)
        assert list(sizes) == [N] * (NF - 1) + [TAIL] and np.array_equal(ref, x.pcm)
        ref.setflags(write=False)
        refs.append(ref)
    return st, refs


def windows_of(st):
    """[(run bytes, frame sizes, fixed block size, first sample, count)], three per stream, and per window
    (stream, first sample, the count it delivers, its frames)."""
    wins, facts = [], []
    for s, x in enumerate(st):
        asked = [(0, 1000 + 37 * s, 3000),                          # of the whole stream: 16 or 17 frames, across a cut
                 (7, 7 * N + 500 + s, 700),                         # of a run that starts at frame 7
                 (NF - 1, (NF - 1) * N + 10, 60 if s % 2 else 200)]  # of the short last frame alone; cut at its end
        for f0, first, count in asked:
            wins.append((x.s[x.off[f0]:], x.fb[f0:], N, first, count))
            got = min(count, TOTAL - first)
            facts.append((s, first, got, (first + got - 1) // N - first // N + 1))
    return wins, facts


@pytest.mark.parametrize("sample_bytes", [4, 2])
def test_three_windows_of_each_of_eight_streams(streams, monkeypatch, sample_bytes):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    st, refs = streams
    wins, facts = windows_of(st)
    cap = sum(w[4] for w in wins)
    dt = np.int16 if sample_bytes == 2 else np.int32
    with V.DecodeSet(like(), 8, V.SET_MD5_OFF) as g:
        before = g.device_batches()
        res, status, decoded, begins = g.decode_windows(wins, cap, sample_bytes)
        assert list(status) == [0] * len(wins)
        want_frames = sum(f[3] for f in facts)
        assert decoded == want_frames < 8 * NF                          # the planner's count, not the streams'
        assert g.device_batches() - before == -(-want_frames // BATCH)
        at = 0
        for (s, first, got, _), r, b in zip(facts, res, begins):
            assert b == at and len(r) == got and r.dtype == dt
            assert np.array_equal(r, refs[s][first:first + got].astype(dt)), (s, first)
            at += got                                                   # back to back, in call order


def test_a_failed_window_keeps_the_room_it_asked_for(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    st, refs = streams
    wins, facts = windows_of(st)
    # a bit in frame 9 of stream 3 (inside its second window) and in frame 20 of stream 5 (inside its first, whose
    # frames are cut between batches); and the header of the short last frame of stream 6, its third window's only one
    hurt = {3 * 3 + 1: (3, 9), 5 * 3: (5, 20), 6 * 3 + 2: (6, NF - 1)}
    wins = [list(w) for w in wins]
    for w, (s, f) in hurt.items():
        x = st[s]
        bad = x.s.copy()
        if f == NF - 1:
            bad[x.off[f] + 2] ^= 0x10                                   # the block-size code: the CRC-8 fails
        else:
            bad[x.off[f + 1] - 4] ^= 0x02
        f0 = {0: 0, 1: 7, 2: NF - 1}[w % 3]
        wins[w][0] = bad[x.off[f0]:]
    cap = sum(w[4] for w in wins)
    out = np.full((cap + 8, 2), -1234567, np.int32)
    with V.DecodeSet(like(), 8, V.SET_MD5_OFF) as g:
        res, status, decoded, begins = g.decode_windows(wins, cap, 4, out=out)
    assert np.all(out[cap:] == -1234567)
    assert [w for w in range(len(wins)) if status[w]] == sorted(hurt)
    assert status[6 * 3 + 2] == V.V_HEADER                              # the planner's: the device was not asked
    at = 0
    for w, ((s, first, got, _), r, b) in enumerate(zip(facts, res, begins)):
        assert b == at
        if w in hurt:
            assert r is None
            at += wins[w][4]                                            # the requested room
        else:
            assert np.array_equal(r, refs[s][first:first + got]), w     # the neighbours, where the counts put them
            at += got


def test_the_sets_state_is_untouched(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    st, refs = streams
    wins, facts = windows_of(st)
    runs = [(s, x.s, x.fb) for s, x in enumerate(st)]

    def message16(vals):
        return np.ascontiguousarray(vals.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :2].tobytes()

    want = [hashlib.md5(message16(r.reshape(-1))).digest() for r in refs]
    for with_windows in (False, True):
        with V.DecodeSet(like(), 8) as g:
            if with_windows:
                # (one window is hurt: a failing window fails no stream)
                bad = [list(w) for w in wins]
                x = st[2]
                b = x.s.copy()
                b[x.off[10] - 4] ^= 0x02
                bad[2 * 3 + 1][0] = b[x.off[7]:]
                res, status, decoded, _ = g.decode_windows(bad)
                assert [w for w in range(len(bad)) if status[w]] == [2 * 3 + 1]
            got = g.decode_runs(runs, 8 * TOTAL)
            for s in range(8):
                assert g.failed(s) is None and np.array_equal(got[s], refs[s])
            assert [g.md5(s) for s in range(8)] == want


def test_bad_arguments_write_nothing(streams):
    st, refs = streams
    x = st[0]
    good = (x.s, x.fb, N, 100, 50)
    with V.DecodeSet(like(), 2, V.SET_MD5_OFF) as g:
        for wins, kw in (([(x.s[:-1], x.fb, N, 100, 50)], {}),                     # the sizes run past the bytes
                         ([good, (x.s, x.fb, N, 100, -1)], {}),                     # a negative count
                         ([good, good], dict(pcm_cap=99)),                          # less room than the counts ask for
                         ([good], dict(sample_bytes=3))):
            out = np.full((128, 2), -77, np.int32)
            with pytest.raises(V.FlakeHipError):
                g.decode_windows(wins, kw.get("pcm_cap", 100), kw.get("sample_bytes", 4), out=out)
            assert np.all(out == -77), (kw, g.last_error())
        res, status, decoded, _ = g.decode_windows([good, good])
        assert decoded == 2 and np.array_equal(res[0], refs[0][100:150]) and np.array_equal(res[1], res[0])
    with V.DecodeSet(like(24), 2, V.SET_MD5_OFF) as g24:
        out = np.full((128, 2), -77, np.int16)
        with pytest.raises(V.FlakeHipError):
            g24.decode_windows([good], 100, 2, out=out)                             # 2-byte samples above 16 bits
        assert np.all(out == -77)
