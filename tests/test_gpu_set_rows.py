"""flake_amd_set_encode_rows (StreamSet.encode_rows): rows of a planar batch on the device through a stream set.  The
contract is the header's: for every stream the frames, the STREAMINFO (device MD5 included), the seek points and the
stream's state afterwards are what StreamSet.encode on the call's whole blocks followed by StreamSet.encode_ragged on its
short blocks give on the numpy-converted samples -- a second set opened the same way does exactly that.  Level 5 and,
under SET_VBS, level 10, both with blocks of 256; FLAKE_AMD_BATCH=4, so that the first call's ten whole blocks span
three chunks and a row's blocks straddle a border.  Then the files go through DecodeSet.decode_windows_rows as float32
and give back the rows that were encoded.  Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_rows_in_kernel import conv

pytestmark = pytest.mark.gpu

V = flake_amd
B, ROW_LEN, BATCH, NSTREAMS, SPACING = 256, 1027, 4, 9, 300
# call 1: (length, stream); stream 7 stays open (two whole blocks) and goes on in call 2
CALL1 = [(0, 0), (1, 1), (255, 2), (256, 3), (257, 4), (768, 5), (785, 6), (512, 7)]
# call 2: stream 7 goes on and ends, stream 3 (one whole block so far) ends; with variable block size a short block ends
# nothing, so there stream 2 (255 samples so far) gets ten more
CALL2 = [(300, 7), (100, 3)]
CALL2_VBS = CALL2 + [(10, 2)]
FORMATS = {"s16-int16": (2, 16, V.ROWS_I16), "s16-float32": (2, 16, V.ROWS_F32),
           "c3x24-int32": (3, 24, V.ROWS_I32), "c3x24-float32": (3, 24, V.ROWS_F32)}
LEVELS = {"level5": (5, 0), "level10-vbs": (10, V.SET_VBS)}
NP_DT = {V.ROWS_I32: np.int32, V.ROWS_I16: np.int16, V.ROWS_F32: np.float32}


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def samples(nrows, ch, bps, seed):
    """[nrows][ch][ROW_LEN] samples of bps bits, the extremes among them."""
    x = V.synth_pcm(nrows, ROW_LEN, ch, bps, first_frame=seed).reshape(nrows, ROW_LEN, ch).transpose(0, 2, 1).astype(np.int64)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    x[:, :, 0] = hi
    x[:, 0, 100] = lo
    x[:, -1, 300] = lo + 1
    return np.ascontiguousarray(x)


def as_rows(x, fmt, bps):
    """The samples as rows of the format: float32 rows lie on the grid, so that they come back from a decode as they are."""
    if fmt == V.ROWS_F32:
        return (x / 2.0 ** (bps - 1)).astype(np.float32)
    return x.astype(NP_DT[fmt])


def open_set(level, flags, ch, bps, verify=False):
    g = V.StreamSet(NSTREAMS, level=level, channels=ch, bits_per_sample=bps, flags=flags, block_size=B)
    g.seekpoints(SPACING)
    if verify:
        g.set_verify(True)
    return g


def host_calls(g, pcm, call):
    """What the contract names, on converted samples pcm [nrows][ch][ROW_LEN] int32: encode on the whole blocks in
    (row, block) order, encode_ragged on the short blocks in row order.  Returns each row's bytes, whole blocks then
    tail."""
    whole, wstream, short, sizes, sstream = [], [], [], [], []
    for r, (n, s) in enumerate(call):
        for b in range(n // B):
            whole.append(pcm[r][:, b * B:(b + 1) * B].T)
            wstream.append(s)
        if n % B:
            short.append(pcm[r][:, n - n % B:n].T)
            sizes.append(n % B)
            sstream.append(s)
    out = [b""] * len(call)
    if whole:
        data, fs = g.encode(np.concatenate(whole), B, wstream)
        at, k = 0, 0
        for r, (n, s) in enumerate(call):
            for _ in range(n // B):
                out[r] += data[at:at + fs[k]].tobytes()
                at += int(fs[k])
                k += 1
    if short:
        data, fs = g.encode_ragged(np.concatenate(short), sizes, sstream)
        at, k = 0, 0
        for r, (n, s) in enumerate(call):
            if n % B:
                out[r] += data[at:at + fs[k]].tobytes()
                at += int(fs[k])
                k += 1
    return out


def state_of(g):
    return [(g.streaminfo_bytes(s), g.get_seekpoints(s)[["sample", "offset", "frame_samples"]].tolist()) for s in range(NSTREAMS)]


_REF = {}


def reference(lname, fname):
    """The two host calls per call of the test, on a set of the test's kind, once per (level, format):
    (the samples of both calls, each call's per-row bytes, the state after each call, device batches of call 1)."""
    key = (lname, fname)
    if key not in _REF:
        (level, flags), (ch, bps, fmt) = LEVELS[lname], FORMATS[fname]
        call2 = CALL2_VBS if flags else CALL2
        x1, x2 = samples(len(CALL1), ch, bps, 3), samples(len(call2), ch, bps, 4)
        with open_set(level, flags, ch, bps) as g:
            p1 = conv(as_rows(x1, fmt, bps), fmt, bps)
            assert np.array_equal(p1, x1)                                   # on the grid: the conversion gives them back
            b1 = host_calls(g, p1, CALL1)
            batches = g.device_batches()
            s1 = state_of(g)
            b2 = host_calls(g, conv(as_rows(x2, fmt, bps), fmt, bps), call2)
            s2 = state_of(g)
        _REF[key] = (x1, x2, b1, b2, s1, s2, batches)
    return _REF[key]


@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify"])
@pytest.mark.parametrize("fname", sorted(FORMATS))
@pytest.mark.parametrize("lname", sorted(LEVELS))
def test_rows_are_the_two_host_calls(monkeypatch, lname, fname, verify):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    (level, flags), (ch, bps, fmt) = LEVELS[lname], FORMATS[fname]
    call2 = CALL2_VBS if flags else CALL2
    x1, x2, want1, want2, state1, state2, batches = reference(lname, fname)
    assert batches == 3 + 1                                                 # three chunks of whole blocks, one of short ones
    t = _torch
    with open_set(level, flags, ch, bps, verify) as g:
        rows1 = t.from_numpy(as_rows(x1, fmt, bps)).cuda()
        got1 = g.encode_rows(rows1, [n for n, _ in CALL1], [s for _, s in CALL1])
        assert g.device_batches() == batches
        for r in range(len(CALL1)):
            assert got1[r] == want1[r], (r, len(got1[r]), len(want1[r]))
        assert got1[0] == b"" and all(len(b) > 0 for b in got1[1:])
        assert state_of(g) == state1

        # refusals: each leaves every stream as it was, which the second call then shows
        rows2 = t.from_numpy(as_rows(x2, fmt, bps)).cuda()
        lens2, str2 = [n for n, _ in call2], [s for _, s in call2]
        refused = [(lens2[:1] + [ROW_LEN + 1] + lens2[2:], str2, "a length above row_len"),
                   (lens2, str2[:1] + [NSTREAMS] + str2[2:], "a stream index outside the set"),
                   (lens2, str2[:1] + [-1] + str2[2:], "a negative stream index"),
                   (lens2[:1] + [-1] + lens2[2:], str2, "a negative length"),
                   (lens2, [7] * len(str2), "two short blocks of one stream in a call")]
        if not flags:
            refused.append((lens2, str2[:1] + [1] + str2[2:], "a block for a stream that a short block has ended"))
        for lens, strs, why in refused:
            with pytest.raises(V.FlakeHipError):
                g.encode_rows(rows2, lens, strs)
            assert g.last_error(), why
            assert state_of(g) == state1, why
        if bps > 16:
            with pytest.raises(V.FlakeHipError):
                g.encode_rows(rows2.to(t.int16), lens2, str2)               # int16 rows above 16 bits
            assert state_of(g) == state1
        with pytest.raises(ValueError):
            g.encode_rows(rows2.cpu(), lens2, str2)                          # not on the set's device
        assert g.encode_rows(rows2[:0], [], []) == []

        got2 = g.encode_rows(rows2, lens2, str2)
        for r in range(len(call2)):
            assert got2[r] == want2[r], r
        assert state_of(g) == state2

        # round trip: fLaC + STREAMINFO + frames of every stream that has samples, decoded as float32 rows
        frames = {s: b"" for s in range(NSTREAMS)}
        audio = {s: [] for s in range(NSTREAMS)}
        for call, x, got in ((CALL1, x1, got1), (call2, x2, got2)):
            for r, (n, s) in enumerate(call):
                frames[s] += got[r]
                audio[s].append(x[r][:, :n])
        files = {s: b"fLaC" + bytes([0x80, 0, 0, 34]) + g.streaminfo_bytes(s) + frames[s] for s in frames if frames[s]}
    assert sorted(files) == list(range(1, 8))
    wins, want = [], []
    for s, data in sorted(files.items()):
        assert data[:4] == b"fLaC" and data[4] & 0x7F == 0
        si, hi = V.read_streaminfo(data[8:42])
        total = sum(a.shape[1] for a in audio[s])
        assert hi == 0 and si.samples == total and si.channels == ch and si.bits_per_sample == bps
        sizes, used = V.index_frames(si, data[42:])
        assert used == len(data) - 42
        wins.append((data[42:], sizes, 0 if flags else B, 0, total))
        row = np.zeros((ch, ROW_LEN), np.float32)
        row[:, :total] = np.concatenate(audio[s], axis=1) / 2.0 ** (bps - 1)
        want.append(row)
    like = V.HostStreaminfo(min_block_size=16 if flags else B, max_block_size=B, sample_rate=44100, channels=ch,
                            bits_per_sample=bps)
    with V.DecodeSet(like, len(wins), V.SET_MD5_OFF) as d:
        back, lengths, status, _ = d.decode_windows_rows(wins, ROW_LEN, t.float32)
    assert list(status) == [0] * len(wins) and lengths.tolist() == [w[4] for w in wins]
    back = back.cpu().numpy()
    for k in range(len(wins)):
        assert np.array_equal(back[k], want[k]), k
        if fmt == V.ROWS_F32:
            # ... which for float32 rows are the very elements that were encoded, padding zero
            src = [as_rows(x, fmt, bps)[r][:, :n] for call, x in ((CALL1, x1), (call2, x2)) for r, (n, s) in enumerate(call)
                   if s == k + 1]
            assert np.array_equal(back[k][:, :wins[k][4]], np.concatenate(src, axis=1))


def test_a_set_that_hashes_on_the_host_is_refused_and_goes_on(monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    ch, bps, fmt = FORMATS["s16-int16"]
    x = samples(2, ch, bps, 5)
    t = _torch
    with V.StreamSet(2, level=5, channels=ch, bits_per_sample=bps, flags=V.SET_MD5_HOST, block_size=B) as g, \
            V.StreamSet(2, level=5, channels=ch, bits_per_sample=bps, flags=V.SET_MD5_HOST, block_size=B) as ref:
        with pytest.raises(V.FlakeHipError):
            g.encode_rows(t.from_numpy(as_rows(x, fmt, bps)).cuda(), [B, B], [0, 1])
        assert "MD5_HOST" in g.last_error()
        pcm = np.concatenate([x[0][:, :B].T, x[1][:, :B].T]).astype(np.int32)
        got, want = g.encode(pcm, B, [0, 1]), ref.encode(pcm, B, [0, 1])
        assert got[0].tobytes() == want[0].tobytes()
        assert [g.streaminfo_bytes(s) for s in (0, 1)] == [ref.streaminfo_bytes(s) for s in (0, 1)]


def test_multiples_of_the_block_size_leave_streams_open_at_any_block_size(monkeypatch):
    """Rows that are whole blocks need no ragged path: a set of blocks above 16384 takes them, and refuses a row with a
    tail before anything is encoded."""
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    n = 16640                                                               # above the ragged path's 16384
    ch, bps, fmt = FORMATS["s16-int16"]
    r = np.random.RandomState(2)
    x = r.randint(-2000, 2000, size=(2, ch, 2 * n)).astype(np.int16)
    t = _torch
    with V.StreamSet(2, level=5, channels=ch, bits_per_sample=bps, block_size=n) as g, \
            V.StreamSet(2, level=5, channels=ch, bits_per_sample=bps, block_size=n) as ref:
        rows = t.from_numpy(x).cuda()
        with pytest.raises(V.FlakeHipError):
            g.encode_rows(rows, [2 * n, n + 1], [0, 1])
        assert "16384" in g.last_error()
        got = g.encode_rows(rows, [2 * n, n], [0, 1])
        pcm = np.concatenate([x[0][:, :n].T, x[0][:, n:].T, x[1][:, :n].T]).astype(np.int32)
        data, fs = ref.encode(pcm, n, [0, 0, 1])
        assert got[0] == data[:fs[0] + fs[1]].tobytes() and got[1] == data[fs[0] + fs[1]:].tobytes()
        assert [g.streaminfo_bytes(s) for s in (0, 1)] == [ref.streaminfo_bytes(s) for s in (0, 1)]
