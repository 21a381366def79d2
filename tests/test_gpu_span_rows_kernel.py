"""K13 alone (fhip_span_rows_from_segments_dev, flake_amd.Encoder.span_rows_from_segments_dev) against numpy: torch tensors
stand for K7's output and its per-segment tables, and the expectation is the delivery rule of include/flakehip_spans.h
written out row by row in numpy (the kernel goes tile by tile).  As in test_gpu_rows_kernel.py the destination and the
source each sit in the middle of a larger tensor of the test's own, filled with a sentinel (the destination) or with
samples (the source): whatever no segment delivers must keep the sentinel -- K13 zeroes nothing -- before, between and
behind the rows, and the table values that lie out of range are chosen so that even an unclamped access would land
inside those tensors and show as a wrong value, not as a fault.  Every comparison is exact and covers the whole tensor."""
import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_rows_kernel import CAP, NP_DT, ROW_GUARD, SENT, SRC_GUARD, conv, handle, source

pytestmark = pytest.mark.gpu

V = flake_amd
TILE = 512
FORMATS = [(V.ROWS_I32, 32), (V.ROWS_I16, 16), (V.ROWS_F32, 24)]
PAIRS = [(7, 1), (1027, 1027), (1027, 513), (1024, 256), (5, 12)]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def nrows_of(count, row_len, hop):
    return min(-(-count // hop), 1 + -(-max(count - row_len, 0) // hop)) if count > 0 else 0


def spans_table():
    """Spans as lists of segments (seg_start, seg_samples, seg_failed, seg_pos): segments of 1, 3, 511, 512, 513 and 1500
    samples, starts on every residue modulo 4, positions 0, 1 and 900 (a row boundary of every pair lies inside that
    tile), two segments of one span that meet inside a row, and a failed segment between two good ones."""
    return [
        [(0, 1500, -1, 0)],                                   # three tiles, the last of 476 samples
        [(1501, 513, -1, 1)],                                 # start 1 mod 4; the span's sample 0 is never delivered
        [(2018, 512, -1, 900)],                               # start 2 mod 4; one whole tile across a row boundary
        [(2531, 511, -1, 0), (3044, 3, -1, 511)],             # start 3 mod 4; the two meet at position 511
        [(3050, 1, -1, 0), (3052, 64, 7, 1), (3117, 3, -1, 65)],
    ]


def flatten(spans, row_len, hop, nrows_for=nrows_of):
    """The per-segment tables (start, samples, failed, pos, row0, nrows), and the rows in all."""
    segs, at = [], 0
    for sp in spans:
        n = nrows_for(max(p + max(m, 0) for _, m, _, p in sp), row_len, hop)
        segs += [(start, m, failed, p, at, n) for start, m, failed, p in sp]
        at += n
    return segs, at


def expected(pcm, segs, nrows, ch, row_len, hop, fmt, bps):
    out = np.full((nrows + 2 * ROW_GUARD, ch, row_len), SENT[fmt], dtype=NP_DT[fmt])
    body = out[ROW_GUARD:ROW_GUARD + nrows]
    for start, m, failed, pos, row0, nr in segs:
        if failed >= 0 or nr < 1 or row0 < 0 or row0 + nr > nrows or pos < 0 or not 0 <= start < CAP:
            continue
        m = min(m, CAP - start)
        for j in range(nr):
            lo, hi = max(pos, j * hop), min(pos + m, j * hop + row_len)
            if hi > lo:
                body[row0 + j, :, lo - j * hop:hi - j * hop] = conv(pcm[start + lo - pos:start + hi - pos], fmt, bps).T
    return out


def run(enc, big_src, segs, nrows, ch, row_len, hop, fmt, over=None, extra_tiles=0):
    """Upload, run K13 on the middles of the two tensors, return (rc, launches, the whole destination)."""
    t = _torch
    src = t.from_numpy(big_src).cuda()
    dst = t.full((nrows + 2 * ROW_GUARD, ch, row_len), SENT[fmt], dtype=getattr(t, NP_DT[fmt].__name__), device="cuda")
    cols = list(zip(*segs))
    start, samples, pos = (t.tensor(cols[i], dtype=t.int64).cuda() for i in (0, 1, 3))
    failed, row0, nr = (t.tensor(cols[i], dtype=t.int32).cuda() for i in (2, 4, 5))
    tiles = np.concatenate([[0], np.cumsum([-(-max(min(m, CAP), 0) // TILE) for m in cols[1]])]).astype(np.int32)
    tile_first = t.from_numpy(tiles).cuda()
    t.cuda.synchronize()
    args = dict(pcm=src[SRC_GUARD:], pcm_cap=CAP, nsegs=len(segs), seg_start=start, seg_samples=samples, seg_failed=failed,
                seg_row0=row0, seg_nrows=nr, seg_pos=pos, tile_first=tile_first, ntiles=int(tiles[-1]) + extra_tiles, hop=hop,
                rows=dst[ROW_GUARD:], nrows=nrows, row_len=row_len, fmt=fmt)
    args.update(over or {})
    rc = enc.span_rows_from_segments_dev(**args)
    launches = enc.last_launches()
    enc.sync()
    return rc, launches, dst.cpu().numpy()


def check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("fmt,bps", FORMATS)
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_every_sample_in_every_row_it_belongs_to(ch, fmt, bps):
    big = source(ch, bps)
    pcm = big[SRC_GUARD:SRC_GUARD + CAP]
    with handle(ch, bps) as enc:
        for row_len, hop in PAIRS:
            segs, nrows = flatten(spans_table(), row_len, hop)
            rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, fmt)
            assert rc == V.OK and launches == ["k_span_rows"], (row_len, hop)
            want = expected(pcm, segs, nrows, ch, row_len, hop, fmt, bps)
            check(got, want, (row_len, hop))
            # what the table is meant to exercise did happen: samples in several rows, sentinels left in place
            body = want[ROW_GUARD:ROW_GUARD + nrows]
            assert (body != SENT[fmt]).any() and (body == SENT[fmt]).any()
            if hop < row_len:
                assert np.array_equal(body[0, :, hop:min(row_len, 2 * hop)], body[1, :, :min(row_len, 2 * hop) - hop])
        # hop 4 under long rows, 40 samples only, the rows the caller's: ten rows, each four samples behind the last
        segs = [(1001, 40, -1, 0, 1, 10)]
        rc, launches, got = run(enc, big, segs, 12, ch, 1027, 4, fmt)
        want = expected(pcm, segs, 12, ch, 1027, 4, fmt, bps)
        assert rc == V.OK and launches == ["k_span_rows"]
        check(got, want, "ten rows of 40 samples")
        assert (want[ROW_GUARD + 10, :, :4] != SENT[fmt]).any() and (want[ROW_GUARD + 10, :, 4:] == SENT[fmt]).all()
        assert (want[ROW_GUARD] == SENT[fmt]).all() and (want[ROW_GUARD + 11] == SENT[fmt]).all()


@pytest.mark.parametrize("fmt,bps", FORMATS)
def test_hostile_tables_leave_every_guard_intact(fmt, bps):
    ch, nrows = 2, 9
    big = source(ch, bps)
    pcm = big[SRC_GUARD:SRC_GUARD + CAP]
    segs = [
        (0, 600, -1, 0, 0, 2),                    # good, beside the others
        (700, 600, -1, 0, nrows, 1),              # rows out of range: the row behind the last
        (700, 600, -1, 0, -1, 2),                 # ... a negative first row
        (700, 600, -1, 0, 7, 3),                  # seg_nrows running past nrows
        (700, 600, -1, 0, 2, 0),                  # no rows, and fewer
        (700, 600, -1, 0, 2, -4),
        (700, 600, -1, 0, 2 ** 31 - 1, 2 ** 31 - 1),
        (700, 600, -1, -3, 2, 1),                 # negative positions
        (700, 600, -1, -(2 ** 62), 2, 1),
        (700, 600, -1, 2 ** 63 - 1, 2, 1),        # a position that no row reaches
        (CAP - 20, 700, -1, 0, 3, 2),             # seg_samples beyond pcm_cap: its last 20
        (CAP + 3, 64, -1, 0, 5, 1),               # a start a few samples past pcm_cap
        (-4, 64, -1, 0, 5, 1),                    # a negative start
        (1400, -5, -1, 0, 5, 1),                  # a negative length
        (1400, 64, 0, 0, 5, 1),                   # failed
        (1500, 100, -1, 640, 6, 2),               # good, behind them: row 6 from column 640 on, row 7 from column 128 on
    ]
    with handle(ch, bps) as enc:
        for row_len, hop in ((1027, 512), (7, 1)):
            rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, fmt, extra_tiles=5)
            assert rc == V.OK and launches == ["k_span_rows"]
            want = expected(pcm, segs, nrows, ch, row_len, hop, fmt, bps)
            check(got, want, (row_len, hop))
            assert (want[ROW_GUARD + 2] == SENT[fmt]).all() and (want[ROW_GUARD + 5] == SENT[fmt]).all()
            assert (want[ROW_GUARD + 8] == SENT[fmt]).all() and (want[ROW_GUARD + 3, :, :20] != SENT[fmt]).any()


def test_invalid_calls_queue_nothing():
    ch, row_len, hop = 2, 1027, 513
    big = source(ch, 16)
    segs, nrows = flatten(spans_table(), row_len, hop)
    with handle(ch, 16) as enc:
        for over in (dict(pcm=None), dict(seg_start=None), dict(seg_samples=None), dict(seg_failed=None),
                     dict(seg_row0=None), dict(seg_nrows=None), dict(seg_pos=None), dict(tile_first=None), dict(rows=None),
                     dict(nsegs=-1), dict(pcm_cap=-1), dict(ntiles=-1), dict(hop=0), dict(hop=-1), dict(hop=2 ** 31),
                     dict(nrows=0), dict(row_len=0), dict(fmt=3), dict(fmt=-1)):
            rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, V.ROWS_I32, over=over)
            assert rc == V.E_INVALID and launches == [], over
            assert (got == SENT[V.ROWS_I32]).all(), over
        for over in (dict(nsegs=0), dict(pcm_cap=0), dict(ntiles=0)):
            rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, V.ROWS_I32, over=over)
            assert rc == V.OK and launches == [] and (got == SENT[V.ROWS_I32]).all(), over
        # hop at its limit is taken: one row per span
        rc, launches, got = run(enc, big, segs, nrows, ch, row_len, 2 ** 31 - 1, V.ROWS_I32)
        assert rc == V.OK and launches == ["k_span_rows"]
        enc.set_pcm_format(V.PCM_S16)
        rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, V.ROWS_I32)
        assert rc == V.E_UNSUPPORTED and launches == [] and (got == SENT[V.ROWS_I32]).all()
    with handle(ch, 24) as enc:
        rc, launches, got = run(enc, source(ch, 24), segs, nrows, ch, row_len, hop, V.ROWS_I16)
        assert rc == V.E_INVALID and launches == [] and (got == SENT[V.ROWS_I16]).all()      # int16 rows above 16 bits


def test_timed_under_its_name():
    ch, fmt, bps, row_len, hop = 3, V.ROWS_F32, 16, 1024, 256
    big = source(ch, bps)
    segs, nrows = flatten(spans_table(), row_len, hop)
    with handle(ch, bps) as enc:
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        rc, launches, got = run(enc, big, segs, nrows, ch, row_len, hop, fmt)
        assert rc == V.OK and enc.kernel_times(reset=True)["k_span_rows"][1] == 1
