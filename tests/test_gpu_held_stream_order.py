"""K11's device entries held to stream order (tests/streamorder.py), as tests/test_gpu_stream_order.py holds the others:
fhip_frame_heads_dev and fhip_gather_frames_dev see what the caller queued on the handle's stream before the call, what
the caller queues afterwards sees their results, and they have stopped reading their inputs by then -- with no host
synchronisation before, between or after.  The cases, the harness' control and the two passes (once, and twice back to
back) are that file's; the witnesses are flacgen's frame numbers and a numpy gather, never a run of the entry itself.

CASES is module-level data that imports without a GPU: tests/test_held_stream_order_cases_cpu.py holds it against
include/flakehip_held.h (every *_dev entry declared there is covered here) and checks the poison conditions on the
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
FIRST_NUMBERS = (3, 40, 90)       # versions A, B, C of the heads case: one geometry (a one-byte number), three answers


class Heads(T.Case):
    """fhip_frame_heads_dev over the 12 VERBATIM frames of one signal, numbered from 3, 40 or 90: the sizes are the same
    in all three versions and every record's number differs.  The offset and size tables are the same throughout."""

    def __init__(self, oracle):
        self.p, self.max_frames = T.P(5, block_size=T.N_DEC), T.NF_DEC
        x = T.signal(T.SEEDS[1])
        self.frames = [[T.verbatim_frame(x[f * T.N_DEC:(f + 1) * T.N_DEC], first + f, False) for f in range(T.NF_DEC)]
                       for first in FIRST_NUMBERS]
        self.fb = T.sizes_of(self.frames[0])
        assert all(T.sizes_of(f).tolist() == self.fb.tolist() for f in self.frames)
        self.stream = [T.as_u8(f) for f in self.frames]
        self.off = np.concatenate([[0], np.cumsum(self.fb)[:-1]]).astype(np.int64)
        self.sig = [self.want(v).tobytes() for v in range(3)]

    def want(self, v):
        out = np.zeros(T.NF_DEC, dtype=V.FRAME_HEAD_DTYPE)
        for f in range(T.NF_DEC):
            # sync, codes, a one-byte number, the CRC-8: six bytes (1152 and 44.1 kHz have codes of their own)
            out[f] = (FIRST_NUMBERS[v] + f, T.N_DEC, 1 | (6 << 8))
        return out

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        stream = Bulk(t, *(self.stream[v] for v in order))
        # the second call of a back-to-back sequence reads the frames in reverse order
        pick = np.arange(T.NF_DEC)[::-1 if variant else 1].copy()
        off, size = T.up(self.off[pick]), T.up(self.fb[pick])
        o = dict(heads=Guarded(t, T.NF_DEC * 16, t.uint8, 0x5A))
        nbytes = int(self.fb.sum())

        def entry(S):
            assert enc.frame_heads_dev(stream.dev, nbytes, off, size, T.NF_DEC, T.N_DEC, o["heads"].win) == V.OK

        want = self.want(order[1])[pick].view(np.uint8)
        return T.Inst([stream], o, entry, dict(heads=T.eq(want, "heads")))


GATHER_FRAMES = ([(5, 700), (3000, 1), (64, 16385), (20000, 33), (17, 15), (40000, 0), (1 << 40, 9), (123, 4096)],
                 [(9, 33), (25000, 4097), (1, 1), (30000, 16385), (-4, 8), (70, 255), (4, 17), (65535, 2)])
GATHER_SRC_BYTES = 65536


class GatherFrames(T.Case):
    """fhip_gather_frames_dev: eight frames of a 64 KiB source, one longer than a wave's round of stores, two that are
    not accepted; the tables are device memory that stays as it is.  Witness: numpy."""

    def __init__(self, oracle):
        self.p, self.max_frames = T.P(5, block_size=192), 16
        r = np.random.RandomState(19)
        self.src = [r.randint(0, 256, size=GATHER_SRC_BYTES).astype(np.uint8) for _ in T.SEEDS]
        self.sig = [self.want(v)[0].tobytes() for v in range(3)]

    @staticmethod
    def accepted(variant):
        return [(s, n) for s, n in GATHER_FRAMES[variant] if n >= 1 and s >= 0 and s + n <= GATHER_SRC_BYTES]

    def total(self, variant=0):
        return sum(n for _, n in self.accepted(variant))

    def want(self, v, variant=0):
        ok = self.accepted(variant)
        dst = np.concatenate([self.src[v][s:s + n] for s, n in ok])
        fb = np.array([n if (s, n) in ok else 0 for s, n in GATHER_FRAMES[variant]], np.int32)
        return dst, fb

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        src = Bulk(t, *(self.src[v] for v in order))
        rows = GATHER_FRAMES[variant]
        f_src, f_len = T.up([r[0] for r in rows], np.int64), T.up([r[1] for r in rows], np.int32)
        total = self.total(variant)
        o = dict(dst=Guarded(t, total, t.uint8, 0x5A), frame_bytes=Guarded(t, len(rows), t.int32, -77))

        def entry(S):
            assert enc.gather_frames_dev(o["dst"].win, total, o["frame_bytes"].win, src.dev, GATHER_SRC_BYTES, f_src, f_len,
                                         len(rows)) == V.OK

        dst, fb = self.want(order[1], variant)
        return T.Inst([src], o, entry, dict(dst=T.eq(dst, "dst"), frame_bytes=T.eq(fb, "frame_bytes")))


CASES = [
    T.Spec("frame_heads", ["fhip_frame_heads_dev"], Heads),
    T.Spec("gather_frames", ["fhip_gather_frames_dev"], GatherFrames),
]


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_entry_is_ordered_on_its_stream(control, oracle, spec):  # noqa: F811
    case = T.built(spec, oracle)
    with case.handle() as enc:
        T.ordered(enc, spec.id, [case.instance(enc)]).assert_clean()


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_back_to_back(control, oracle, spec):  # noqa: F811
    """The entry twice in a row behind one gate, on inputs B1 then B2 with different tables into separate outputs: the
    second call reuses the handle's workspace while the first may still be pending."""
    case = T.built(spec, oracle)
    with case.handle() as enc:
        calls = [case.instance(enc, (0, 1, 2)), case.instance(enc, (1, 2, 0), variant=1)]
        T.ordered(enc, spec.id + " twice", calls).assert_clean()
