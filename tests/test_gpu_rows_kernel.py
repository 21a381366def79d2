"""K10 alone (fhip_rows_from_segments_dev, flake_amd.Encoder.rows_from_segments_dev) against numpy: torch tensors stand for
K7's output and its per-segment tables, and the expectation is the delivery rule of include/flakehip.h written out in
numpy.  The destination and the source each sit in the middle of a larger tensor of the test's own, filled with a
sentinel (the destination) or with samples (the source): whatever no segment delivers must keep the sentinel -- K10
zeroes nothing -- and the table values that lie out of range are chosen so that even an unclamped access would land
inside those tensors and show as a wrong value, not as a fault.  Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_decode_segments import Stream

pytestmark = pytest.mark.gpu

V = flake_amd
CAP = 4096                        # samples per channel of the source that K10 is told about
SRC_GUARD = 1024                  # samples on either side of it
ROW_GUARD = 2                     # rows on either side of the destination
NROWS = 12
NP_DT = {V.ROWS_I32: np.int32, V.ROWS_I16: np.int16, V.ROWS_F32: np.float32}
SENT = {V.ROWS_I32: -1234567, V.ROWS_I16: -1234, V.ROWS_F32: 12345.5}


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def handle(ch, bps):
    return V.Encoder(V.level_params(5, channels=ch, bits_per_sample=bps, block_size=192, variable_block_size=0), max_frames=4)


def conv(x, fmt, bps):
    """What include/flakehip.h defines for sample x."""
    if fmt == V.ROWS_F32:
        return x.astype(np.float32) * np.float32(2.0 ** -(bps - 1))
    return x.astype(NP_DT[fmt])


def source(ch, bps, seed=3):
    """[SRC_GUARD + CAP + SRC_GUARD][ch] samples of bps bits; the extremes, +-1, +-2 (and 0) lead the part K10 sees."""
    r = np.random.RandomState(seed + 16 * ch + bps)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    big = r.randint(lo, hi + 1, size=(CAP + 2 * SRC_GUARD, ch), dtype=np.int64)
    special = np.array([1, -1, 2, -2, hi, lo, 0, hi - 1, lo + 1, hi // 3], dtype=np.int64)       # (hi = 2^31 - 1 at 32 bits)
    flat = big[SRC_GUARD:].reshape(-1)
    flat[:len(special)] = special
    return big.astype(np.int32)


def segments(row_len):
    """(seg_start, seg_samples, seg_failed, seg_row, seg_col) per segment: lengths 0, 1, 63, 64, 65 and 1025 at starts
    that are and are not multiples of 4 samples, segments adjoining in one row, clipping at the row's end, the two ways
    of not being delivered, and the values out of range."""
    return [
        (0, 1025, -1, 0, 0),                  # three tiles, the last of one sample; start a multiple of 4
        (1025, 1025, -1, 1, 2),               # start 1 mod 4; fills row_len 1027 exactly, is clipped by row_len 1024
        (2050, 63, -1, 2, 0),                 # three segments adjoining in row 2
        (2113, 64, -1, 2, 63),
        (2177, 65, -1, 2, 127),
        (2242, 1, -1, 3, 5),
        (2243, 0, -1, 4, 0),                  # nothing
        (2244, 64, -1, 5, 3),                 # start a multiple of 4, column not
        (2308, 63, -1, 5, 100),
        (2371, 65, -1, -1, 0),                # seg_row -1: not delivered
        (2436, 64, 3, 6, 0),                  # seg_failed >= 0: not delivered
        (2500, 65, -1, 7, row_len - 10),      # clipped by the row's end: 10 samples
        (2600, 64, -1, NROWS, 0),             # out of range: the row behind the last
        (2700, 64, -1, 8, -3),                # ... a negative column
        (2800, 64, -1, 8, row_len),           # ... a column behind the row
        (CAP + 3, 64, -1, 9, 0),              # ... a start a few samples past pcm_cap
        (CAP - 20, 500, -1, 10, 0),           # ... more samples than the source holds: its last 20
        (2900, -5, -1, 11, 0),                # ... a negative length
        (-4, 64, -1, 11, 0),                  # ... a negative start
    ]


def expected(pcm, segs, ch, row_len, fmt, bps):
    out = np.full((NROWS + 2 * ROW_GUARD, ch, row_len), SENT[fmt], dtype=NP_DT[fmt])
    body = out[ROW_GUARD:ROW_GUARD + NROWS]
    for start, n, failed, row, col in segs:
        if failed >= 0 or not 0 <= row < NROWS or not 0 <= col < row_len or not 0 <= start < CAP:
            continue
        m = min(n, row_len - col, CAP - start)
        if m > 0:
            body[row, :, col:col + m] = conv(pcm[start:start + m], fmt, bps).T
    return out


def run(enc, big_src, segs, ch, row_len, fmt, nsegs=None, over=None):
    """Upload, run K10 on the middles of the two tensors, return (rc, launches, the whole destination)."""
    t = _torch
    src = t.from_numpy(big_src).cuda()
    dst = t.full((NROWS + 2 * ROW_GUARD, ch, row_len), SENT[fmt], dtype=getattr(t, NP_DT[fmt].__name__), device="cuda")
    cols = list(zip(*segs))
    start, samples, col = (t.tensor(cols[i], dtype=t.int64).cuda() for i in (0, 1, 4))
    failed, row = (t.tensor(cols[i], dtype=t.int32).cuda() for i in (2, 3))
    t.cuda.synchronize()
    args = dict(pcm=src[SRC_GUARD:], pcm_cap=CAP, nsegs=len(segs) if nsegs is None else nsegs, seg_start=start,
                seg_samples=samples, seg_failed=failed, seg_row=row, seg_col=col, rows=dst[ROW_GUARD:], nrows=NROWS,
                row_len=row_len, fmt=fmt)
    args.update(over or {})
    rc = enc.rows_from_segments_dev(**args)
    launches = enc.last_launches()
    enc.sync()
    return rc, launches, dst.cpu().numpy()


FORMATS = [(V.ROWS_I32, 24), (V.ROWS_I32, 32), (V.ROWS_I16, 8), (V.ROWS_I16, 16),
           (V.ROWS_F32, 8), (V.ROWS_F32, 16), (V.ROWS_F32, 24), (V.ROWS_F32, 32)]


@pytest.mark.parametrize("fmt,bps", FORMATS)
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_every_segment_where_the_tables_put_it(ch, fmt, bps):
    big = source(ch, bps)
    pcm = big[SRC_GUARD:SRC_GUARD + CAP]
    if fmt == V.ROWS_F32:                                                  # the values the conversion is defined on
        lead = conv(pcm.reshape(-1)[:6], fmt, bps)
        assert list(lead[:4]) == [2.0 ** -(bps - 1), -2.0 ** -(bps - 1), 2.0 ** -(bps - 2), -2.0 ** -(bps - 2)]
        assert lead[5] == -1.0 and (lead[4] == 1.0 if bps == 32 else lead[4] == 1.0 - 2.0 ** -(bps - 1))
    with handle(ch, bps) as enc:
        for row_len in (1027, 1024):
            segs = segments(row_len)
            rc, launches, got = run(enc, big, segs, ch, row_len, fmt)
            assert rc == V.OK and launches == ["k_window_rows"]
            want = expected(pcm, segs, ch, row_len, fmt, bps)
            assert got.dtype == want.dtype
            assert np.array_equal(got[:ROW_GUARD], want[:ROW_GUARD]) and np.array_equal(got[-ROW_GUARD:], want[-ROW_GUARD:])
            for r in range(NROWS):
                assert np.array_equal(got[ROW_GUARD + r], want[ROW_GUARD + r]), (row_len, r)
            # what the table is meant to exercise did happen: whole rows, a clipped one, sentinels left in place
            body = want[ROW_GUARD:ROW_GUARD + NROWS]
            assert not (body[0, :, :1025] == SENT[fmt]).all() and (body[0, :, 1025:] == SENT[fmt]).all()
            assert (body[7, :, :row_len - 10] == SENT[fmt]).all() and (body[[4, 6, 8, 9, 11]] == SENT[fmt]).all()


def test_the_clipped_table_is_read_inside_nsegs():
    """nsegs below the tables' length: the segments behind it are not delivered."""
    ch, fmt, bps, row_len = 2, V.ROWS_I32, 16, 1027
    big = source(ch, bps)
    segs = segments(row_len)
    with handle(ch, bps) as enc:
        rc, launches, got = run(enc, big, segs, ch, row_len, fmt, nsegs=2)
    assert rc == V.OK and launches == ["k_window_rows"]
    assert np.array_equal(got, expected(big[SRC_GUARD:SRC_GUARD + CAP], segs[:2], ch, row_len, fmt, bps))


def test_invalid_calls_queue_nothing():
    ch, row_len = 2, 1027
    big = source(ch, 16)
    segs = segments(row_len)
    with handle(ch, 16) as enc:
        for over in (dict(pcm=None), dict(seg_start=None), dict(seg_samples=None), dict(seg_failed=None),
                     dict(seg_row=None), dict(seg_col=None), dict(rows=None), dict(nsegs=-1), dict(pcm_cap=-1),
                     dict(nrows=0), dict(row_len=0), dict(fmt=3), dict(fmt=-1)):
            rc, launches, got = run(enc, big, segs, ch, row_len, V.ROWS_I32, over=over)
            assert rc == V.E_INVALID and launches == [], over
            assert (got == SENT[V.ROWS_I32]).all(), over
        rc, launches, got = run(enc, big, segs, ch, row_len, V.ROWS_I32, nsegs=0)
        assert rc == V.OK and launches == [] and (got == SENT[V.ROWS_I32]).all()
        enc.set_pcm_format(V.PCM_S16)
        rc, launches, got = run(enc, big, segs, ch, row_len, V.ROWS_I32)
        assert rc == V.E_UNSUPPORTED and launches == [] and (got == SENT[V.ROWS_I32]).all()
    with handle(ch, 24) as enc:
        rc, launches, got = run(enc, source(ch, 24), segs, ch, row_len, V.ROWS_I16)
        assert rc == V.E_INVALID and launches == [] and (got == SENT[V.ROWS_I16]).all()      # int16 rows above 16 bits


def test_timed_under_its_name_and_zeroing():
    ch, fmt, bps, row_len = 3, V.ROWS_F32, 16, 1027
    big = source(ch, bps)
    with handle(ch, bps) as enc:
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        rc, launches, got = run(enc, big, segments(row_len), ch, row_len, fmt)
        assert rc == V.OK and enc.kernel_times(reset=True)["k_window_rows"][1] == 1
        # fhip_rows_zero_dev: rows 3 .. 8 of a sentinel-filled destination, and nothing else
        t = _torch
        dst = t.full((NROWS + 2 * ROW_GUARD, ch, row_len), SENT[fmt], dtype=t.float32, device="cuda")
        t.cuda.synchronize()
        assert enc.rows_zero_dev(dst[ROW_GUARD:], NROWS, row_len, fmt, 3, 5) == V.OK and enc.last_launches() == []
        for first, count in ((-1, 1), (0, -1), (NROWS, 1), (NROWS - 1, 2)):
            assert enc.rows_zero_dev(dst[ROW_GUARD:], NROWS, row_len, fmt, first, count) == V.E_INVALID
        enc.sync()
        z = dst.cpu().numpy()
        assert (z[ROW_GUARD + 3:ROW_GUARD + 8] == 0).all()
        assert (z[:ROW_GUARD + 3] == SENT[fmt]).all() and (z[ROW_GUARD + 8:] == SENT[fmt]).all()


def test_behind_the_window_decode_on_one_stream():
    """fhip_decode_frames_windows_rows: K7's window mode, then K10 on what it left on the device -- the rows hold what
    fhip_decode_frames_windows delivers, the other outputs are that entry's, and the launch list is its list with K10 at
    the end."""
    n, row_len = 64, 131
    with V.Encoder(V.level_params(5, block_size=n, variable_block_size=0), max_frames=32) as enc:
        a, b = Stream(enc, 5, n, 0, 1), Stream(enc, 4, n, 7, 3)
        s = np.concatenate([a.s, b.s])
        fb = np.concatenate([a.fb, b.fb]).astype(np.int32)
        sf, num = [0, 5, 9], [0, 7]
        skip, take = [10, 70], [131, 100]
        rc, pcm, nsm, recs, summary, s_start, s_samples, s_failed, _ = enc.decode_frames_windows(
            s, fb, 512, sf, skip, take, seg_number=num)
        assert rc == V.OK and list(s_samples) == [131, 100] and enc.last_launches()[-1] != "k_window_rows"
        window_list = enc.last_launches()
        t = _torch
        for fmt, dt in ((V.ROWS_I32, t.int32), (V.ROWS_I16, t.int16), (V.ROWS_F32, t.float32)):
            dst = t.full((3, 2, row_len), SENT[fmt], dtype=dt, device="cuda")
            t.cuda.synchronize()
            got = enc.decode_frames_windows_rows(s, fb, 512, sf, skip, take, [2, 0], [0, 31], dst, 3, row_len, fmt,
                                                 seg_number=num)
            assert got[0] == V.OK and got[1] is None and got[2] == nsm
            assert enc.last_launches() == window_list + ["k_window_rows"]
            assert np.array_equal(got[3], recs) and np.array_equal(got[4], summary)
            assert list(got[5]) == list(s_start) and list(got[6]) == list(s_samples) and list(got[7]) == list(s_failed)
            want = np.full((3, 2, row_len), SENT[fmt], dtype=NP_DT[fmt])
            want[2, :, :131] = conv(pcm[s_start[0]:s_start[0] + 131], fmt, 16).T
            want[0, :, 31:131] = conv(pcm[s_start[1]:s_start[1] + 100], fmt, 16).T
            assert np.array_equal(dst.cpu().numpy(), want), fmt
        enc.set_pcm_format(V.PCM_S16)
        dst = t.full((3, 2, row_len), SENT[V.ROWS_I16], dtype=t.int16, device="cuda")
        t.cuda.synchronize()
        got = enc.decode_frames_windows_rows(s, fb, 512, sf, skip, take, [2, 0], [0, 31], dst, 3, row_len, V.ROWS_I16,
                                             seg_number=num)
        assert got[0] == V.E_UNSUPPORTED and enc.last_launches() == [] and (dst.cpu().numpy() == SENT[V.ROWS_I16]).all()
