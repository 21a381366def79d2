"""K12's device entry held to stream order (tests/streamorder.py), as tests/test_gpu_stream_order.py holds the others and
tests/test_gpu_held_stream_order.py the held entries: fhip_pcm_from_rows_dev sees what the caller queued on the handle's
stream before the call, what the caller queues afterwards sees its result, and it has stopped reading the rows by then
-- with no host synchronisation before, between or after.  The cases, the harness' control and the two passes (once,
and twice back to back) are that file's; the witness is the conversion rule of include/flakehip_rows_in.h in numpy.

CASES is module-level data that imports without a GPU: tests/test_rows_in_stream_order_cases_cpu.py holds it against
include/flakehip_rows_in.h (every *_dev entry declared there is covered here) and checks the poison conditions on the
CPU."""
import numpy as np
import pytest
import torch as _torch

import flake_amd
import test_gpu_stream_order as T
from streamorder import Bulk, Guarded
from test_gpu_stream_order import control, torch  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

V = flake_amd
NROWS, ROW_LEN, BPS = 4, 1027, 16
# (row, col, dst, count); the second table is what the second call of the back-to-back sequence brings, so that a host
# image rewritten under a pending copy would show.  One piece is longer than a K12 tile of 1024 samples.
ROWS_IN_PIECES = ([(2, 0, 0, 1027), (0, 5, 1027, 1), (3, 100, 1028, 333), (1, 3, 1361, 250)],
                  [(1, 700, 0, 250), (3, 0, 250, 1027), (0, 1026, 1277, 1), (2, 9, 1278, 333)])
ROWS_IN_TOTAL = 1611


def rows_in_conv(e, bps):
    """include/flakehip_rows_in.h's FHIP_ROWS_F32 rule, exact in float64."""
    x = np.rint(e.astype(np.float64) * 2.0 ** (bps - 1))
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(x, -2.0 ** (bps - 1), 2.0 ** (bps - 1) - 1).astype(np.int32)


class RowsIn(T.Case):
    """fhip_pcm_from_rows_dev: four pieces of float32 stereo rows whose length puts the channel planes at different
    offsets modulo 16 bytes; the piece table goes through the handle's host image.  Witness: numpy."""

    def __init__(self, oracle):
        self.p, self.max_frames = T.P(5, block_size=192), 4
        r = np.random.RandomState(23)
        self.src = [(r.randint(-2 ** 15, 2 ** 15, size=(NROWS, 2, ROW_LEN)) / 2.0 ** 15).astype(np.float32) for _ in T.SEEDS]
        self.sig = [self.want(v).tobytes() for v in range(3)]
        assert all(sum(p[3] for p in ps) == ROWS_IN_TOTAL for ps in ROWS_IN_PIECES)

    def want(self, v, variant=0):
        out = np.zeros((ROWS_IN_TOTAL, 2), np.int32)
        for row, col, dst, count in ROWS_IN_PIECES[variant]:
            out[dst:dst + count] = rows_in_conv(self.src[v][row][:, col:col + count], BPS).T
        return out

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        rows = Bulk(t, *(self.src[v].reshape(-1) for v in order))
        o = dict(dst=Guarded(t, ROWS_IN_TOTAL * 2, t.int32, -1234567))
        pieces = V.row_pieces(ROWS_IN_PIECES[variant])

        def entry(S):
            assert enc.pcm_from_rows_dev(o["dst"].win, ROWS_IN_TOTAL, rows.dev, NROWS, ROW_LEN, V.ROWS_F32, pieces) == V.OK

        return T.Inst([rows], o, entry, dict(dst=T.eq(self.want(order[1], variant), "dst")))


CASES = [
    T.Spec("pcm_from_rows", ["fhip_pcm_from_rows_dev"], RowsIn),
]


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_entry_is_ordered_on_its_stream(control, oracle, spec):  # noqa: F811
    case = T.built(spec, oracle)
    with case.handle() as enc:
        T.ordered(enc, spec.id, [case.instance(enc)]).assert_clean()


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_back_to_back(control, oracle, spec):  # noqa: F811
    """The entry twice in a row behind one gate, on inputs B1 then B2 with different tables into separate outputs: the
    second call reuses the handle's piece-table image while the first may still be pending."""
    case = T.built(spec, oracle)
    with case.handle() as enc:
        calls = [case.instance(enc, (0, 1, 2)), case.instance(enc, (1, 2, 0), variant=1)]
        T.ordered(enc, spec.id + " twice", calls).assert_clean()
