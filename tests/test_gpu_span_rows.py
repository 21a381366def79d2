"""Span rows (DecodeSet.decode_span_rows / held_span_rows) against the entries they stand beside: a span's rows and lengths
are, exactly, what held_windows_rows (decode_windows_rows for the runs form) returns for the windows
(id, first + j * hop, min(row_len, count - j * hop)), j < R -- the parent's entry, not the code under test -- and, as a
second witness, numpy slices of the PCM that was encoded.  The four kinds of stream of test_gpu_held_windows.py with
FLAKE_AMD_BATCH=3, so that device batches cut every long span; spans over the whole stream and beyond its end, inside
it, of one sample, of count 0, behind the end and on a stream held twice; overlapping, adjoining and spaced rows.  The
point of the feature is held as a condition: the whole-stream span hands every frame to the decoder once, the windows
hand over more.  Damage fails a span whole and alone; refusals leave the destination untouched.  Every comparison is
exact."""
import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
from test_gpu_held_windows import BATCH, KINDS, as_runs, damaged, made, open_set

pytestmark = pytest.mark.gpu

V = flake_amd


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(autouse=True)
def small_batches(monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))


def pcm_of(kind, seed=0):
    """The samples made(kind, seed) encoded."""
    level, ch, bps, n, nb, tail = KINDS[kind]
    return V.synth_pcm(nb + 1, n, ch, bps, first_frame=seed).reshape(-1, ch)[:nb * n + tail]


def spans_for(m, a, b):
    """[(held id, first sample, count)] on held streams a and b (b holds the same bytes as a)."""
    n, t = m.n, m.total
    return [(a, 0, t + 1000),                 # the whole stream, the count beyond its end
            (a, n + 7, 5 * n),                # inside it, across six frames: more than a device batch
            (a, 0, 1),
            (a, 100, 0),                      # count 0: no row
            (a, t + 5, 10),                   # behind the end: one row of nothing
            (b, n + 7, 5 * n)]                # the same stream, held twice


def windows_of(spans, row_len, hop):
    """The composition: every row of every span as a window of its own."""
    return [(i, first + j * hop, min(row_len, count - j * hop))
            for i, first, count in spans for j in range(V.span_rows_count(count, row_len, hop))]


def first_rows(spans, row_len, hop):
    return np.concatenate([[0], np.cumsum([V.span_rows_count(c, row_len, hop) for _, _, c in spans])]).astype(np.int64)


def slices(pcm, spans, row_len, hop):
    """The second witness: the rows (int32) and lengths as numpy slices of the samples that were encoded."""
    rows, lens = [], []
    for _, first, count in spans:
        x = pcm[first:first + count]
        for j in range(V.span_rows_count(count, row_len, hop)):
            part = x[j * hop:j * hop + row_len]
            row = np.zeros((pcm.shape[1], row_len), dtype=np.int32)
            row[:, :len(part)] = part.T
            rows.append(row)
            lens.append(len(part))
    return np.stack(rows), lens


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_span_rows_are_the_windows_rows_of_their_rows(kind):
    m = made(kind)
    pcm = pcm_of(kind)
    g, ids, table = open_set(m, [m.bytes, m.bytes])
    with g:
        spans = spans_for(m, *ids)
        for row_len, hop in ((1000, 500), (m.n, m.n), (300, 700)):
            wins = windows_of(spans, row_len, hop)
            first = first_rows(spans, row_len, hop)
            R = int(first[-1])
            assert R == len(wins) > 10
            for dtype in (_torch.int32, _torch.float32, _torch.int16):
                if (dtype == _torch.int16 and m.bps > 16) or (dtype != _torch.int32 and (row_len, hop) != (1000, 500)):
                    continue
                wrows, wlen, wstatus, wdecoded = g.held_windows_rows(wins, row_len, dtype)
                assert not any(wstatus)
                out = _torch.full((R + 2, m.ch, row_len), 77, dtype=dtype, device="cuda")
                before = g.device_batches()
                rows, lens, span_first, status, decoded = g.held_span_rows(spans, row_len, hop, out=out)
                batches = g.device_batches() - before
                assert rows.dtype == dtype and rows.shape == (R, m.ch, row_len) and list(status) == [0] * len(spans)
                assert list(span_first) == list(first)
                assert lens.tolist() == wlen.tolist()
                assert np.array_equal(rows.cpu().numpy(), wrows.cpu().numpy()), (row_len, hop, dtype)
                assert (out[R:].cpu().numpy() == 77).all()                         # rows behind the call's are not touched
                assert batches == -(-decoded // BATCH)
                # (rows with gaps between them may leave frames out that the span still decodes)
                assert decoded < wdecoded or hop > row_len
                if dtype == _torch.int32:
                    srows, slens = slices(pcm, spans, row_len, hop)
                    assert lens.tolist() == slens and np.array_equal(rows.cpu().numpy(), srows), (row_len, hop)
                    # the runs form, against decode_windows_rows in the same way
                    rrows, rlen, rfirst, rstatus, rdecoded = g.decode_span_rows(as_runs(spans, table), row_len, hop, dtype)
                    crows, clen, cstatus, _ = g.decode_windows_rows(as_runs(wins, table), row_len, dtype)
                    assert list(rfirst) == list(first) and list(rstatus) == [0] * len(spans) and rdecoded == decoded
                    assert rlen.tolist() == clen.tolist() == slens and not any(cstatus)
                    assert np.array_equal(rrows.cpu().numpy(), crows.cpu().numpy())
                    assert np.array_equal(rrows.cpu().numpy(), srows)
            # the lengths say what they should: a full row, the stream's last samples, nothing behind the end
            assert lens[0] == row_len and lens[int(first[1]) - 1] == min(row_len, max(0, m.total - (int(first[1]) - 1) * hop))
            assert lens[int(first[2])] == 1 and first[3] == first[4] and lens[int(first[4])] == 0


def test_every_frame_is_decoded_once():
    """The point of the feature: the whole-stream span at (1000, 500) hands each of the stream's 15 frames to K7 once, in
    ceil(15 / 3) device batches; the same rows asked as windows hand over more."""
    m = made("stereo16_fixed1152")
    g, ids, table = open_set(m, [m.bytes])
    with g:
        frames = g.held_info(ids[0])[0]
        assert frames == 15
        spans = [(ids[0], 0, m.total)]
        wins = windows_of(spans, 1000, 500)
        assert len(wins) == 33
        before = g.device_batches()
        rows, lens, first, status, decoded = g.held_span_rows(spans, 1000, 500, _torch.int32)
        batches = g.device_batches() - before
        wrows, wlen, wstatus, wdecoded = g.held_windows_rows(wins, 1000, _torch.int32)
        print(f"frames handed to K7: {decoded} for the span in {batches} batches, {wdecoded} for its {len(wins)} rows as windows")
        assert decoded == frames and batches == -(-frames // BATCH)
        assert wdecoded > decoded
        assert list(first) == [0, 33] and list(status) == [0] and lens.tolist() == wlen.tolist()
        assert np.array_equal(rows.cpu().numpy(), wrows.cpu().numpy())
        rrows, rlen, _, rstatus, rdecoded = g.decode_span_rows(as_runs(spans, table), 1000, 500, _torch.int32)
        assert rdecoded == frames and list(rstatus) == [0] and np.array_equal(rrows.cpu().numpy(), wrows.cpu().numpy())


def test_damage_fails_a_span_whole_and_alone():
    """The copy with frame 9's first subframe header made invalid under a good CRC-16: K8 takes the frame and K7 refuses
    it.  A span over the whole copy fails -- rows zero, lengths -1, a status -- although its first batches delivered; a
    good span in the same call is intact, and so is a span of the copy that ends before frame 9."""
    m = made("stereo16_fixed1152")
    with V.DecodeSet(m.si, 1, V.SET_MD5_OFF) as g0:
        sizes = g0.index([m.bytes])[0][0]
    syntax_bytes = damaged(m, sizes)[4]
    n = m.n
    g, ids, table = open_set(m, [m.bytes, syntax_bytes])
    with g:
        good, syntax = ids
        assert g.held_info(syntax)[0] == 15
        spans = [(good, 2 * n, 3 * n), (syntax, 0, m.total), (good, 0, m.total), (syntax, 100, 9 * n - 200)]
        for row_len, hop in ((1000, 500), (300, 700)):
            first = first_rows(spans, row_len, hop)
            for held in (True, False):
                if held:
                    rows, lens, span_first, status, _ = g.held_span_rows(spans, row_len, hop, _torch.int32)
                else:
                    rows, lens, span_first, status, _ = g.decode_span_rows(as_runs(spans, table), row_len, hop, _torch.int32)
                got, lens = rows.cpu().numpy(), lens.numpy()
                assert list(span_first) == list(first)
                assert status[1] != 0 and [status[0], status[2], status[3]] == [0, 0, 0]
                assert not got[first[1]:first[2]].any() and lens[first[1]:first[2]].tolist() == [-1] * int(first[2] - first[1])
                ok = [spans[0], spans[2], spans[3]]
                wrows, wlen, wstatus, _ = g.held_windows_rows(windows_of(ok, row_len, hop), row_len, _torch.int32)
                assert not any(wstatus)
                keep = np.r_[0:first[1], first[2]:first[4]]
                assert np.array_equal(got[keep], wrows.cpu().numpy()) and lens[keep].tolist() == wlen.tolist()
                assert got[first[2]:first[3]].any() and got[first[3]:].any()


def test_refusals_leave_the_destination_untouched():
    m = made("stereo16_fixed1152")
    g, ids, table = open_set(m, [m.bytes])
    row_len, hop = 1000, 500
    with g:
        spans = [(ids[0], 0, 3000), (ids[0], 500, 1200)]
        R = int(first_rows(spans, row_len, hop)[-1])
        assert R == 5 + 2

        def refused(call, rows, dtype=_torch.int32):
            out = _torch.full((rows, m.ch, row_len), 77, dtype=dtype, device="cuda")
            with pytest.raises(V.FlakeHipError):
                call(out)
            assert (out.cpu().numpy() == 77).all()

        for held in (True, False):
            def ask(s, h, out, rl=row_len):
                if held:
                    return g.held_span_rows(s, rl, h, out=out)
                return g.decode_span_rows(as_runs(s, table), rl, h, out=out)
            refused(lambda out: ask(spans, 0, out), R + 1)                         # hop 0
            refused(lambda out: ask(spans, -3, out), R + 1)
            refused(lambda out: ask(spans, 2 ** 31, out), R + 1)
            refused(lambda out: ask(spans, hop, out), R - 1)                       # rows_cap one short
            refused(lambda out: ask([(ids[0], 0, -1)], hop, out), R)               # a negative count
            # exactly enough is enough, and the row behind the call's stays as it was
            out = _torch.full((R + 1, m.ch, row_len), 77, dtype=_torch.int32, device="cuda")
            rows, lens, first, status, _ = ask(spans, hop, out)
            assert rows.shape[0] == R and lens.tolist() == [1000, 1000, 1000, 1000, 1000, 1000, 700]
            assert (out[R:].cpu().numpy() == 77).all() and (out[:R].cpu().numpy() != 77).any()
        refused(lambda out: g.held_span_rows([(ids[0], 0, 100), (len(ids), 0, 100)], row_len, hop, out=out), 4)   # an unknown id
        refused(lambda out: g.held_span_rows([(-1, 0, 100)], row_len, hop, out=out), 4)
        # no span at all: no row, and nothing touched
        out = _torch.full((2, m.ch, row_len), 77, dtype=_torch.int32, device="cuda")
        rows, lens, first, status, decoded = g.held_span_rows([], row_len, hop, out=out)
        assert rows.shape[0] == 0 and list(first) == [0] and decoded == 0 and (out.cpu().numpy() == 77).all()
    m24 = made("eight24_256")
    g, ids, table = open_set(m24, [m24.bytes])
    with g:
        out = _torch.full((8, m24.ch, row_len), 77, dtype=_torch.int16, device="cuda")
        with pytest.raises(V.FlakeHipError):
            g.held_span_rows([(ids[0], 0, 1000)], row_len, hop, out=out)           # int16 rows at 24 bits
        with pytest.raises(V.FlakeHipError):
            g.decode_span_rows(as_runs([(ids[0], 0, 1000)], table), row_len, hop, out=out)
        assert (out.cpu().numpy() == 77).all()
