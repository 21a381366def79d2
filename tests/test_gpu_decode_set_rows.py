"""flake_amd_decode_set_windows_rows (DecodeSet.decode_windows_rows): the windows of flake_amd_decode_set_windows as a padded
planar batch [window][channel][time] that stays on the device.  The shapes are test_gpu_decode_set_windows.py's: eight
stereo 16-bit streams of 39 frames of 192 and a last one of 100, three windows per stream, FLAKE_AMD_BATCH=16 so that
batches are cut inside windows.  The expectation is what decode_windows returns on a set of the same kind, placed into a
zero [W][C][T] numpy array and converted as include/flakehip.h defines; every comparison is exact."""
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
NP_DT = {_torch.int32: np.int32, _torch.int16: np.int16, _torch.float32: np.float32}
SENT = {_torch.int32: -1234567, _torch.int16: -1234, _torch.float32: 12345.5}


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def like(bps=16, ch=2, n=N):
    return V.HostStreaminfo(min_block_size=n, max_block_size=n, sample_rate=44100, channels=ch, bits_per_sample=bps)


def conv(x, dtype, bps):
    if dtype == _torch.float32:
        return x.astype(np.float32) * np.float32(2.0 ** -(bps - 1))
    return x.astype(NP_DT[dtype])


def planar(res, nwin, ch, row_len, dtype, bps):
    """decode_windows' per-window samples [n][ch] in a zero [W][C][T] array; (array, lengths)."""
    want = np.zeros((nwin, ch, row_len), dtype=NP_DT[dtype])
    lengths = []
    for w, r in enumerate(res):
        lengths.append(-1 if r is None else len(r))
        if r is not None and len(r):
            want[w, :, :len(r)] = conv(r, dtype, bps).T
    return want, lengths


@pytest.fixture(scope="module")
def streams():
    with flake_amd.Encoder(P(5, block_size=N, variable_block_size=0), max_frames=NF) as enc:
        return [Stream(enc, NF - 1, N, 0, 10 + s, tail=TAIL) for s in range(8)]


def windows_of(st):
    """[(run bytes, frame sizes, fixed block size, first sample, count)], three per stream."""
    wins = []
    for s, x in enumerate(st):
        for f0, first, count in ((0, 1000 + 37 * s, 3000),                  # of the whole stream: across a cut
                                 (7, 7 * N + 500 + s, 700),                 # of a run that starts at frame 7
                                 (NF - 1, (NF - 1) * N + 10, 60 if s % 2 else 200)):    # the short last frame; cut at its end
            wins.append((x.s[x.off[f0]:], x.fb[f0:], N, first, count))
    return wins


def hurt(st, wins):
    """The existing test's three corruptions: a bit in frame 9 of stream 3 (inside its second window) and in frame 20 of
    stream 5 (inside its first, whose frames are cut between batches, so part of its row has been written); and the
    header of the short last frame of stream 6, its third window's only one.  Returns (windows, the hurt ones)."""
    bad_of = {3 * 3 + 1: (3, 9), 5 * 3: (5, 20), 6 * 3 + 2: (6, NF - 1)}
    wins = [list(w) for w in wins]
    for w, (s, f) in bad_of.items():
        x = st[s]
        bad = x.s.copy()
        if f == NF - 1:
            bad[x.off[f] + 2] ^= 0x10                                       # the block-size code: the CRC-8 fails
        else:
            bad[x.off[f + 1] - 4] ^= 0x02
        f0 = {0: 0, 1: 7, 2: NF - 1}[w % 3]
        wins[w][0] = bad[x.off[f0]:]
    return wins, sorted(bad_of)


@pytest.fixture(scope="module")
def reference(streams):
    """decode_windows (the host sink) on the good and on the hurt windows, once: (res, status, decoded, batches) each."""
    import os
    old = os.environ.get("FLAKE_AMD_BATCH")
    os.environ["FLAKE_AMD_BATCH"] = str(BATCH)
    try:
        out = {}
        good = windows_of(streams)
        for name, wins in (("good", good), ("hurt", hurt(streams, good)[0])):
            with V.DecodeSet(like(), 8, V.SET_MD5_OFF) as g:
                before = g.device_batches()
                res, status, decoded, _ = g.decode_windows(wins)
                out[name] = (res, list(status), decoded, g.device_batches() - before)
    finally:
        if old is None:
            del os.environ["FLAKE_AMD_BATCH"]
        else:
            os.environ["FLAKE_AMD_BATCH"] = old
    return out


@pytest.mark.parametrize("row_len", [3000, 3001])
@pytest.mark.parametrize("dtype", [_torch.int32, _torch.int16, _torch.float32])
def test_rows_are_the_host_windows_placed_and_converted(streams, reference, monkeypatch, dtype, row_len):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    wins = windows_of(streams)
    res, status, decoded, batches = reference["good"]
    assert batches > 1
    want, lengths = planar(res, len(wins), 2, row_len, dtype, 16)
    with V.DecodeSet(like(), 8, V.SET_MD5_OFF) as g:
        before = g.device_batches()
        rows, got_len, got_status, got_decoded = g.decode_windows_rows(wins, row_len, dtype)
        assert g.device_batches() - before == batches
    assert rows.is_cuda and rows.dtype == dtype and tuple(rows.shape) == (len(wins), 2, row_len)
    assert got_len.dtype == _torch.int64 and not got_len.is_cuda and got_len.tolist() == lengths
    assert list(got_status) == status == [0] * len(wins) and got_decoded == decoded
    got = rows.cpu().numpy()
    for w in range(len(wins)):
        assert np.array_equal(got[w], want[w]), w
    assert (got[0, :, 3000:] == 0).all() and (got[1, :, 700:] == 0).all()       # the padding is zero


@pytest.mark.parametrize("dtype", [_torch.int32, _torch.int16, _torch.float32])
def test_a_failed_window_is_a_zero_row(streams, reference, monkeypatch, dtype):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    wins, bad = hurt(streams, windows_of(streams))
    res, status, decoded, batches = reference["hurt"]
    assert [w for w in range(len(wins)) if status[w]] == bad and all(res[w] is None for w in bad)
    row_len = 3001
    want, lengths = planar(res, len(wins), 2, row_len, dtype, 16)
    # out= with two rows more than the call's: sentinels everywhere beforehand
    out = _torch.full((len(wins) + 2, 2, row_len), SENT[dtype], dtype=dtype, device="cuda")
    with V.DecodeSet(like(), 8, V.SET_MD5_OFF) as g:
        rows, got_len, got_status, got_decoded = g.decode_windows_rows(wins, row_len, out=out)
    assert rows.data_ptr() == out.data_ptr() and tuple(rows.shape) == (len(wins), 2, row_len)
    assert got_len.tolist() == lengths and [lengths[w] for w in bad] == [-1, -1, -1]
    assert list(got_status) == status and got_decoded == decoded
    got = out.cpu().numpy()
    assert (got[len(wins):] == SENT[dtype]).all()                          # the extra rows are untouched
    for w in range(len(wins)):
        assert np.array_equal(got[w], want[w]), w
        assert (got[w] == 0).all() == (w in bad), w                        # exactly those rows are zero, the others intact


def test_windows_that_deliver_nothing_are_zero_rows(streams):
    x = streams[0]
    wins = [(x.s, x.fb, N, 100, 50),
            (x.s, x.fb, N, TOTAL, 40),                                      # begins behind its run's end
            (x.s, x.fb, N, 300, 0),                                         # count 0
            (x.s, x.fb, N, TOTAL - 7, 64)]                                  # the run ends inside it: 7 samples
    with V.DecodeSet(like(), 2, V.SET_MD5_OFF) as g:
        res, status, _, _ = g.decode_windows(wins)
        out = _torch.full((4, 2, 64), 12345.5, dtype=_torch.float32, device="cuda")
        rows, lengths, got_status, _ = g.decode_windows_rows(wins, 64, out=out)
        # no window at all: nothing to write, nothing refused
        none = g.decode_windows_rows([], 64)
        assert tuple(none[0].shape) == (0, 2, 64) and none[1].tolist() == []
    want, want_len = planar(res, 4, 2, 64, _torch.float32, 16)
    assert lengths.tolist() == want_len == [50, 0, 0, 7] and list(got_status) == list(status) == [0, 0, 0, 0]
    got = rows.cpu().numpy()
    assert np.array_equal(got, want) and (got[1] == 0).all() and (got[2] == 0).all() and (got[3, :, 7:] == 0).all()


def test_refusals_write_nothing(streams):
    x = streams[0]
    good = (x.s, x.fb, N, 100, 50)
    with V.DecodeSet(like(), 2, V.SET_MD5_OFF) as g:
        for wins, row_len in (([good, (x.s, x.fb, N, 100, 65)], 64),        # a count above row_len
                              ([(x.s[:-1], x.fb, N, 100, 50)], 64),          # the sizes run past the bytes
                              ([good, (x.s, x.fb, N, 100, -1)], 64)):        # a negative count
            out = _torch.full((2, 2, row_len), -1234567, dtype=_torch.int32, device="cuda")
            with pytest.raises(V.FlakeHipError):
                g.decode_windows_rows(wins, row_len, out=out[:len(wins)])
            assert (out.cpu().numpy() == -1234567).all(), g.last_error()
        with pytest.raises(V.FlakeHipError):
            g.decode_windows_rows([good], 0)                                 # row_len < 1
        for out in (_torch.zeros((1, 2, 64), dtype=_torch.int32),                                     # not on the device
                    _torch.zeros((1, 2, 65), dtype=_torch.int32, device="cuda"),                      # another row_len
                    _torch.zeros((1, 2, 128), dtype=_torch.int32, device="cuda")[:, :, ::2]):         # not contiguous
            with pytest.raises(ValueError):
                g.decode_windows_rows([good], 64, out=out)
        with pytest.raises(ValueError):
            g.decode_windows_rows([good], 64, dtype=_torch.float16)
    with V.DecodeSet(like(24), 2, V.SET_MD5_OFF) as g24:
        out = _torch.full((1, 2, 64), -1234, dtype=_torch.int16, device="cuda")
        with pytest.raises(V.FlakeHipError):
            g24.decode_windows_rows([good], 64, out=out)                     # int16 rows on a 24-bit set
        assert (out.cpu().numpy() == -1234).all()


@pytest.mark.parametrize("ch,bps", [(1, 24), (8, 8)])
def test_other_formats_in_float32(monkeypatch, ch, bps):
    """Two streams of six frames of 64, batches of four frames: windows across frames and across a batch cut."""
    monkeypatch.setenv("FLAKE_AMD_BATCH", "4")
    n = 64
    with flake_amd.Encoder(P(5, channels=ch, bits_per_sample=bps, block_size=n, variable_block_size=0), max_frames=8) as enc:
        st = [Stream(enc, 6, n, 0, 20 + s) for s in range(2)]
    wins = [(st[0].s, st[0].fb, n, 30, 300), (st[1].s[st[1].off[2]:], st[1].fb[2:], n, 2 * n + 5, 97), (st[1].s, st[1].fb, n, 0, 1)]
    with V.DecodeSet(like(bps, ch, n), 2, V.SET_MD5_OFF) as g:
        res, status, decoded, _ = g.decode_windows(wins)
        rows, lengths, got_status, got_decoded = g.decode_windows_rows(wins, 301)
    assert rows.dtype == _torch.float32 and list(status) == list(got_status) == [0, 0, 0] and decoded == got_decoded
    for w, (x, first, count) in enumerate(((st[0], 30, 300), (st[1], 2 * n + 5, 97), (st[1], 0, 1))):
        assert np.array_equal(res[w], x.pcm[first:first + count])           # (the reference is the encoder's input)
    want, want_len = planar(res, 3, ch, 301, _torch.float32, bps)
    assert lengths.tolist() == want_len == [300, 97, 1]
    assert np.array_equal(rows.cpu().numpy(), want)
    assert np.abs(want).max() <= 1.0


def test_the_sets_state_is_untouched(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    wins, bad = hurt(streams, windows_of(streams))
    runs = [(s, x.s, x.fb) for s, x in enumerate(streams)]
    digests = []
    for with_rows in (False, True):
        with V.DecodeSet(like(), 8) as g:
            if with_rows:
                _, lengths, _, _ = g.decode_windows_rows(wins, 3000)
                assert [w for w in range(len(wins)) if lengths[w] < 0] == bad
            got = g.decode_runs(runs, 8 * TOTAL)
            for s, x in enumerate(streams):
                assert g.failed(s) is None and np.array_equal(got[s], x.pcm)
            digests.append([g.md5(s) for s in range(8)])
    assert digests[0] == digests[1] and None not in digests[0]
    want = hashlib.md5(np.ascontiguousarray(streams[0].pcm.astype("<i2")).tobytes()).digest()
    assert digests[1][0] == want
