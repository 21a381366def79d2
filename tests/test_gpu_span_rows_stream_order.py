"""fhip_span_rows_from_segments_dev held to stream order (tests/streamorder.py), as test_gpu_stream_order.py holds the K10
entry: poison A in the PCM, a gate on the stream, the real PCM B copied in behind the gate, fhip_rows_zero_dev and the
K13 entry, snapshots of the rows and poison C into the PCM, all on one non-default torch stream with no host
synchronisation before, between or after -- once, and twice back to back into separate rows.  The witness is the source
PCM placed by numpy with the delivery rule of include/flakehip_spans.h, never a synchronous run of the entry."""
import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
from streamorder import Bulk, Guarded
from test_gpu_stream_order import SEEDS, Case, Inst, P, control, eq, ordered, rows_conv, signal, up  # noqa: F401

pytestmark = pytest.mark.gpu

V = flake_amd
ROW_LEN, HOP = 700, 300
# two spans: 1000 samples in two segments that meet at position 700 -- inside the second row --, and 650 samples from position 5
STARTS, COUNTS, POS = [0, 700, 1000], [700, 300, 650], [0, 700, 5]
ROW0, NROWS_OF = [0, 0, 2], [2, 2, 1]
NROWS = 3
TILE_FIRST = [0, 2, 3, 5]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def span_rows_of(pcm, fmt):
    rows = np.zeros((NROWS, 2, ROW_LEN), np.float32 if fmt == V.ROWS_F32 else np.int32)
    for start, m, pos, row0, nr in zip(STARTS, COUNTS, POS, ROW0, NROWS_OF):
        for j in range(nr):
            lo, hi = max(pos, j * HOP), min(pos + m, j * HOP + ROW_LEN)
            if hi > lo:
                rows[row0 + j, :, lo - j * HOP:hi - j * HOP] = rows_conv(pcm[start + lo - pos:start + hi - pos], fmt).T
    return rows


class SpanRows(Case):
    """fhip_rows_zero_dev + fhip_span_rows_from_segments_dev alone: the PCM is the input, K7's tables are fixed."""

    def __init__(self, fmt):
        self.fmt, self.p, self.max_frames = fmt, P(5, block_size=192), 4
        self.pcm = [signal(s, 1700) for s in SEEDS]
        self.sig = [span_rows_of(x, fmt).tobytes() for x in self.pcm]
        assert len(set(self.sig)) == 3

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t, fmt = _torch, self.fmt
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        dt = t.float32 if fmt == V.ROWS_F32 else t.int32
        o = dict(rows=Guarded(t, NROWS * 2 * ROW_LEN, dt, 12345.5 if fmt == V.ROWS_F32 else -1234567))
        st, cn, fl = up(STARTS, np.int64), up(COUNTS, np.int64), up([-1, -1, -1], np.int32)
        row0, nr, pos, tf = up(ROW0, np.int32), up(NROWS_OF, np.int32), up(POS, np.int64), up(TILE_FIRST, np.int32)

        def entry(S):
            assert enc.rows_zero_dev(o["rows"].win, NROWS, ROW_LEN, fmt, 0, NROWS) == V.OK
            assert enc.span_rows_from_segments_dev(pcm.dev, 1700, 3, st, cn, fl, row0, nr, pos, tf, TILE_FIRST[-1], HOP,
                                                   o["rows"].win, NROWS, ROW_LEN, fmt) == V.OK

        return Inst([pcm], o, entry, dict(rows=eq(span_rows_of(self.pcm[order[1]], fmt), "rows")))


_BUILT = {}


def case_of(fmt):
    if fmt not in _BUILT:
        _BUILT[fmt] = SpanRows(fmt)
    return _BUILT[fmt]


@pytest.mark.parametrize("fmt", [V.ROWS_I32, V.ROWS_F32], ids=["i32", "f32"])
def test_entry_is_ordered_on_its_stream(control, fmt):
    case = case_of(fmt)
    with case.handle() as enc:
        ordered(enc, f"span_rows_{fmt}", [case.instance(enc)]).assert_clean()


@pytest.mark.parametrize("fmt", [V.ROWS_I32, V.ROWS_F32], ids=["i32", "f32"])
def test_back_to_back(control, fmt):
    case = case_of(fmt)
    with case.handle() as enc:
        calls = [case.instance(enc, (0, 1, 2)), case.instance(enc, (1, 2, 0), variant=1)]
        ordered(enc, f"span_rows_{fmt} twice", calls).assert_clean()
