"""K12 alone (fhip_pcm_from_rows_dev, flake_amd.Encoder.pcm_from_rows_dev) against numpy: a torch tensor stands for the
caller's planar batch, and the expectation is the conversion rule of include/flakehip_rows_in.h written out in numpy
(float64, where it is exact).  The destination sits in the middle of a larger tensor filled with a sentinel and the rows
in the middle of a larger tensor of samples: whatever no piece covers must keep the sentinel.  A table that the host
check takes never reaches the kernel out of range, so every refusal is held to its return code, an empty launch list and
an untouched destination.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as _torch

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
NROWS = 6
ROW_GUARD = 2                     # rows on either side of the rows K12 is told about
DST_GUARD = 64                    # samples on either side of the destination
SENT = -1234567
NP_DT = {V.ROWS_I32: np.int32, V.ROWS_I16: np.int16, V.ROWS_F32: np.float32}
COUNTS = (1, 3, 4, 5, 1023, 1024, 1025)


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def handle(ch, bps):
    return V.Encoder(V.level_params(5, channels=ch, bits_per_sample=bps, block_size=192, variable_block_size=0), max_frames=4)


def conv(e, fmt, bps):
    """What include/flakehip_rows_in.h defines for element e."""
    if fmt != V.ROWS_F32:
        return e.astype(np.int32)
    x = np.rint(e.astype(np.float64) * 2.0 ** (bps - 1))
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(x, -2.0 ** (bps - 1), 2.0 ** (bps - 1) - 1).astype(np.int64).astype(np.int32)


def specials(bps):
    """The float32 inputs the rule is defined on, with what each must give."""
    h = 2 ** (bps - 1)
    f = np.float32
    vals = [(0.0, 0), (-0.0, 0), (1.0, h - 1), (-1.0, -h), (1.5, h - 1), (-1.5, -h),
            (np.nextafter(f(1), f(0)), h - 1 if bps <= 24 else h - 128),
            (f(1e-40), 0), (f(-1e-40), 0), (np.inf, h - 1), (-np.inf, -h), (np.nan, 0),
            (f(3e38), h - 1), (f(-3e38), -h)]
    # every on-grid extreme and its neighbours
    for k in (h - 1, h - 2, -h, -h + 1, 1, -1):
        if bps <= 24:
            vals.append((k / h, k))
    if bps <= 24:
        # ties (k + 0.5) / 2^(b-1) go to the even neighbour; the last one rounds up to 2^(b-1) and clamps
        for k, want in ((0, 0), (1, 2), (2, 2), (3, 4), (-1, 0), (-2, -2), (-3, -2), (-4, -4), (h - 3, h - 2),
                        (h - 2, h - 2), (h - 1, h - 1), (-h, -h)):
            vals.append(((k + 0.5) / h, want))
    e = np.array([v for v, _ in vals], dtype=np.float32)
    assert all(float(a) == float(b) or (np.isnan(a) and np.isnan(b)) for a, (b, _) in zip(e, vals))      # representable
    return e, np.array([w for _, w in vals], dtype=np.int64)


def source(ch, fmt, bps, row_len, seed=7):
    """[ROW_GUARD + NROWS + ROW_GUARD][ch][row_len] elements; for float32 the special values lead every row from column 4
    on, rotated by the channel."""
    r = np.random.RandomState(seed + 16 * ch + bps + fmt)
    shape = (NROWS + 2 * ROW_GUARD, ch, row_len)
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if fmt != V.ROWS_F32:
        big = r.randint(lo, hi + 1, size=shape, dtype=np.int64)
        big[:, :, 4:10] = [hi, lo, 0, -1, 1, hi - 1]
        return big.astype(NP_DT[fmt])
    grid = r.randint(lo, hi + 1, size=shape, dtype=np.int64) / 2.0 ** (bps - 1)
    free = r.uniform(-1.2, 1.2, size=shape)
    big = np.where(r.randint(0, 2, size=shape) == 1, grid, free).astype(np.float32)
    e, _ = specials(bps)
    for c in range(ch):
        big[:, c, 4:4 + len(e)] = np.roll(e, c)
    return big


def pieces_for(row_len):
    """(row, col, dst, count): every count of COUNTS at every column 0..3 mod 4, four rounds with a piece of one to
    four samples between them so that every count also lands at every dst 0..3 mod 4; consecutive pieces come from different rows, so
    the runs of short pieces put adjoining pieces of different rows inside one lane's four samples."""
    out, nominal, at, i = [], [], 0, 0
    for rnd in range(4):
        for count in COUNTS:
            for cm in range(4):
                col = cm if count > 5 else cm + 4 * (1 + (i % 7))
                n = min(count, row_len - col)
                out.append((i % NROWS, col, at, n))
                nominal.append(count)
                at += n
                i += 1
        pad = (rnd + 1 - at) % 4 or 4                                       # the next round starts at dst = rnd + 1 mod 4
        out.append(((i + 3) % NROWS, row_len - pad, at, pad))               # (up to the row's last column)
        nominal.append(0)
        at += pad
        i += 1
    return out, at, nominal


def expected(rows, pieces, total, ch, fmt, bps):
    out = np.full((total + 2 * DST_GUARD, ch), SENT, dtype=np.int32)
    for row, col, dst, n in pieces:
        out[DST_GUARD + dst:DST_GUARD + dst + n] = conv(rows[row][:, col:col + n], fmt, bps).T
    return out


def run(enc, big, pieces, total, ch, fmt, row_len, over=None, raw_pieces=None):
    """Upload, run K12 on the middles of the two tensors, return (rc, launches, the whole destination)."""
    t = _torch
    src = t.from_numpy(big).cuda()
    dst = t.full((total + 2 * DST_GUARD, ch), SENT, dtype=t.int32, device="cuda")
    t.cuda.synchronize()
    args = dict(dst=dst[DST_GUARD:], dst_cap=total, rows=src[ROW_GUARD:], nrows=NROWS, row_len=row_len, fmt=fmt,
                pieces=V.row_pieces(pieces) if raw_pieces is None else raw_pieces)
    args.update(over or {})
    rc = enc.pcm_from_rows_dev(**args)
    launches = enc.last_launches()
    enc.sync()
    return rc, launches, dst.cpu().numpy()


FORMATS = [(V.ROWS_I32, 8), (V.ROWS_I32, 16), (V.ROWS_I32, 24), (V.ROWS_I32, 32), (V.ROWS_I16, 8), (V.ROWS_I16, 16),
           (V.ROWS_F32, 8), (V.ROWS_F32, 16), (V.ROWS_F32, 24), (V.ROWS_F32, 32)]


def test_the_piece_table_covers_what_it_is_meant_to():
    for row_len in (1027, 1024):
        pieces, total, nominal = pieces_for(row_len)
        assert total == sum(p[3] for p in pieces)
        for count in COUNTS:
            mine = [p for p, c in zip(pieces, nominal) if c == count]
            # (a piece that would leave the row is cut at its end: 1025 samples fit row_len 1027 from columns 0 to 2)
            assert all(p[3] == min(count, row_len - p[1]) for p in mine)
            assert count > row_len or any(p[3] == count for p in mine)
            assert {p[1] % 4 for p in mine} == {0, 1, 2, 3}, (row_len, count)
            assert {p[2] % 4 for p in mine} == {0, 1, 2, 3}, (row_len, count)
        assert all(0 <= r < NROWS and c >= 0 and c + n <= row_len and n >= 1 for r, c, _, n in pieces)
        # adjoining pieces of different rows inside one aligned group of four destination samples
        assert any(a[0] != b[0] and a[2] // 4 == b[2] // 4 for a, b in zip(pieces, pieces[1:]))


def test_the_rule_on_the_special_values():
    for bps in (8, 16, 24, 32):
        e, want = specials(bps)
        assert conv(e, V.ROWS_F32, bps).tolist() == want.tolist(), bps


@pytest.mark.parametrize("fmt,bps", FORMATS)
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_every_piece_where_the_table_puts_it(ch, fmt, bps):
    with handle(ch, bps) as enc:
        for row_len in (1027, 1024):
            big = source(ch, fmt, bps, row_len)
            pieces, total, _ = pieces_for(row_len)
            rc, launches, got = run(enc, big, pieces, total, ch, fmt, row_len)
            assert rc == V.OK and launches == ["k_rows_to_pcm"]
            want = expected(big[ROW_GUARD:ROW_GUARD + NROWS], pieces, total, ch, fmt, bps)
            assert (want[:DST_GUARD] == SENT).all() and (want[-DST_GUARD:] == SENT).all()
            assert np.array_equal(got[:DST_GUARD], want[:DST_GUARD]) and np.array_equal(got[-DST_GUARD:], want[-DST_GUARD:])
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (row_len, int(bad[0]) - DST_GUARD, got[bad[0]], want[bad[0]])
            if fmt == V.ROWS_F32:
                # the special values were converted: a long piece from column 0 of row 0 covers them
                e, w = specials(bps)
                p = next(p for p in pieces if p[0] == 0 and p[1] == 0 and p[3] >= 1023)
                at = DST_GUARD + p[2] + 4
                assert got[at:at + len(e), 0].tolist() == w.tolist()


def test_a_destination_that_is_not_16_byte_aligned_and_a_capacity_above_the_total():
    ch, fmt, bps, row_len = 3, V.ROWS_F32, 16, 1027
    big = source(ch, fmt, bps, row_len)
    pieces, total, _ = pieces_for(row_len)
    t = _torch
    with handle(ch, bps) as enc:
        src = t.from_numpy(big).cuda()
        dst = t.full((total + 2 * DST_GUARD + 1, ch), SENT, dtype=t.int32, device="cuda")
        t.cuda.synchronize()
        win = dst.reshape(-1)[DST_GUARD * ch + 1:]                           # 4 bytes past a 16-byte boundary
        assert win.data_ptr() % 16 == 4
        rc = enc.pcm_from_rows_dev(win, total + 5, src[ROW_GUARD:], NROWS, row_len, fmt, V.row_pieces(pieces))
        assert rc == V.OK and enc.last_launches() == ["k_rows_to_pcm"]
        enc.sync()
        got = dst.cpu().numpy().reshape(-1)
        want = np.full(got.shape, SENT, np.int32)
        body = expected(big[ROW_GUARD:ROW_GUARD + NROWS], pieces, total, ch, fmt, bps)[DST_GUARD:DST_GUARD + total]
        want[DST_GUARD * ch + 1:DST_GUARD * ch + 1 + total * ch] = body.reshape(-1)
        assert np.array_equal(got, want)


def test_invalid_calls_queue_nothing():
    ch, fmt, row_len = 2, V.ROWS_I32, 1027
    big = source(ch, fmt, 16, row_len)
    good = [(0, 0, 0, 10), (1, 5, 10, 20), (2, 1000, 30, 27)]
    total = 57
    bad_tables = {
        "count 0": [(0, 0, 0, 10), (1, 5, 10, 0), (2, 0, 10, 47)],
        "count negative": [(0, 0, 0, 10), (1, 5, 10, -1), (2, 0, 9, 48)],
        "a gap": [(0, 0, 0, 10), (1, 5, 11, 46)],
        "an overlap": [(0, 0, 0, 10), (1, 5, 9, 48)],
        "not sorted": [(1, 5, 10, 47), (0, 0, 0, 10)],
        "does not start at 0": [(0, 0, 1, 56)],
        "row negative": [(-1, 0, 0, 57)],
        "row behind the last": [(NROWS, 0, 0, 57)],
        "column negative": [(0, -1, 0, 57)],
        "columns past the row": [(0, row_len - 56, 0, 57)],
        "column past the row": [(0, row_len, 0, 1), (0, 0, 1, 56)],
        "total above dst_cap": [(0, 0, 0, 58)],
    }
    with handle(ch, 16) as enc:
        rc, launches, got = run(enc, big, good, total, ch, fmt, row_len)
        assert rc == V.OK and launches == ["k_rows_to_pcm"]
        assert np.array_equal(got, expected(big[ROW_GUARD:ROW_GUARD + NROWS], good, total, ch, fmt, 16))
        for why, table in bad_tables.items():
            rc, launches, got = run(enc, big, table, total, ch, fmt, row_len)
            assert rc == V.E_INVALID and launches == [], why
            assert (got == SENT).all(), why
        for over in (dict(dst=None), dict(rows=None), dict(dst_cap=-1), dict(dst_cap=total - 1), dict(nrows=0), dict(nrows=-1),
                     dict(nrows=2), dict(row_len=0), dict(row_len=-5), dict(row_len=1026), dict(fmt=3), dict(fmt=-1)):
            rc, launches, got = run(enc, big, good, total, ch, fmt, row_len, over=over)
            assert rc == V.E_INVALID and launches == [], over
            assert (got == SENT).all(), over
        # a null table with pieces to read, a negative piece count and a null fhip_rows_in: past the Python view
        dst = _torch.full((total, ch), SENT, dtype=_torch.int32, device="cuda")
        src = _torch.from_numpy(big).cuda()
        _torch.cuda.synchronize()
        ri = V.RowsIn(src[ROW_GUARD:].data_ptr(), NROWS, fmt, row_len)
        tab = V.row_pieces(good)
        for args in ((dst.data_ptr(), total, C.byref(ri), None, 3), (dst.data_ptr(), total, C.byref(ri), tab.ctypes.data, -1),
                     (dst.data_ptr(), total, None, tab.ctypes.data, 3)):
            assert enc.lib.fhip_pcm_from_rows_dev(enc._h, *args) == V.E_INVALID and enc.last_launches() == [], args[2:]
        enc.sync()
        assert (dst.cpu().numpy() == SENT).all()
        # no pieces: nothing is queued
        rc, launches, got = run(enc, big, [], total, ch, fmt, row_len)
        assert rc == V.OK and launches == [] and (got == SENT).all()
        enc.set_pcm_format(V.PCM_S16)
        rc, launches, got = run(enc, big, good, total, ch, fmt, row_len)
        assert rc == V.E_UNSUPPORTED and launches == [] and (got == SENT).all()
    with handle(ch, 24) as enc:
        rc, launches, got = run(enc, source(ch, V.ROWS_I16, 16, row_len), good, total, ch, V.ROWS_I16, row_len)
        assert rc == V.E_INVALID and launches == [] and (got == SENT).all()      # int16 rows above 16 bits


def test_timed_under_its_name():
    ch, fmt, bps, row_len = 3, V.ROWS_F32, 16, 1027
    big = source(ch, fmt, bps, row_len)
    pieces, total, _ = pieces_for(row_len)
    with handle(ch, bps) as enc:
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        rc, launches, got = run(enc, big, pieces, total, ch, fmt, row_len)
        assert rc == V.OK and enc.kernel_times(reset=True)["k_rows_to_pcm"][1] == 1
