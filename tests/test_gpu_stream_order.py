"""Every device entry held to stream order (tests/streamorder.py): what the caller queued on the handle's stream before
the call is seen by the call, what it queues afterwards sees the call's results, and the call has stopped reading its
inputs by then -- with no host synchronisation before, between or after.

Each case passes through streamorder.run_ordered once: poison A in the inputs, a gate on the stream, the real input B
copied in behind the gate, the call, snapshots of the outputs and poison C into the inputs, all on one non-default torch
stream.  The witnesses are those of the synchronous tests of each entry -- the oracle's encode_frame and
flake_encode_frame() loop, the source PCM and numpy placement, hashlib, flacgen's frame table -- never a synchronous
run of the entry itself.  A, B and C are valid inputs of one geometry (FLAC streams are flacgen frames with VERBATIM
subframes only, whose sizes depend on the geometry alone), so a wrong order gives a wrong answer and nothing worse.

CASES is module-level data that imports without a GPU: tests/test_stream_order_cases_cpu.py holds it against the header
(every *_dev entry is covered here or excluded below with a reason) and checks the poison conditions on the CPU.

fhip_prepare_ahead is not here: the header says it is deliberately NOT ordered after the handle's stream, and
tests/test_gpu_ahead.py owns that contract.
"""
import ctypes as C
import functools
import hashlib
import time

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flacgen
import flake_amd
import streamorder as SO
from streamorder import Bulk, Guarded

pytestmark = pytest.mark.gpu

V = flake_amd
P = flake_amd.level_params
SEEDS = (101, 202, 303)          # the signals behind versions A, B, C
N_DEC, NF_DEC = 1152, 12         # the decode, verify and index cases: 12 frames of 1152
FIRST = 3                        # the first frame number of the fixed-block encodes
OK_REC = (0, -1, -1, -1)         # fhip_verify_rec of a good frame

EXCLUDED = {
    "fhip_frames_packed_gather": "synchronises the handle's stream before it returns (as the uploads do); its kernel "
                                 "and table upload are fhip_gather_spans_dev's (run_gather), which is covered",
}


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(scope="session")
def control():
    """The harness must bite before any case means anything: the unordered stand-in is caught, the ordered one passes.
    Every ordering test depends on this fixture and fails with it."""
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    try:
        reps = SO.control_catches_unordered_copy(_torch)
        caught = [r for r in reps if r.failures]
        assert caught, (f"harness control: a copy on a second stream without wait_stream went unnoticed on "
                        f"{len(reps)} side streams; no ordering test of this file means anything")
        assert all(step in (6, 7) for r in caught for step, _, _ in r.failures)
        SO.control_passes_ordered_copy(_torch).assert_clean()
        yield {"side_streams_tried": len(reps)}
    finally:
        SO.write_log()


# ---- shared CPU data ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def signal(seed, nsamples=N_DEC * NF_DEC, ch=2, bps=16):
    x = flacgen.test_signal(nsamples, ch, bps, seed=seed)
    x.setflags(write=False)
    return x


def verbatim_frame(block, number, vbs):
    return flacgen.frame(block, number, 16, 44100, [dict(kind="verbatim")] * block.shape[1], vbs=vbs)


@functools.lru_cache(maxsize=None)
def verbatim_frames(seed, vbs=False):
    """The 12 frames of signal(seed), VERBATIM subframes only, numbered from 0 by frame (or by sample: vbs)."""
    x = signal(seed)
    return tuple(verbatim_frame(x[f * N_DEC:(f + 1) * N_DEC], f * N_DEC if vbs else f, vbs) for f in range(NF_DEC))


def as_u8(frames):
    return np.frombuffer(b"".join(frames), np.uint8).copy()


def sizes_of(frames):
    return np.array([len(f) for f in frames], np.int32)


def eq(want, what):
    """A checker for streamorder: the whole output equals want."""
    want = np.asarray(want).reshape(-1)

    def check(host):
        assert host.dtype == want.dtype and host.shape == want.shape, (what, host.dtype, host.shape)
        bad = np.nonzero(host != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} values differ, first at {int(bad[0])}: {host[bad[0]]} != {want[bad[0]]}"
    return check


def prefix(want, what):
    """... its first len(want) elements equal want (what lies behind them is unspecified)."""
    want = np.asarray(want).reshape(-1)

    def check(host):
        got = host[:want.size]
        assert got.dtype == want.dtype, (what, got.dtype)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{what}: {bad.size} values differ, first at {int(bad[0])}"
    return check


def up(a, dtype=None):
    """A table that is the same in all three versions: uploaded once, before the harness drains the device."""
    return _torch.from_numpy(np.array(a, dtype=dtype)).cuda()


class Inst:
    """One prepared call: its bulk inputs, guarded outputs, the entry and what version B must give."""

    def __init__(self, inputs, outputs, entry, expected):
        self.inputs, self.outputs, self.entry, self.expected = inputs, outputs, entry, expected


class Case:
    """CPU side of a case: p / max_frames / verify of its handle, sig[v] = what the witness gives for version v (bytes;
    pairwise different), and instance(enc, order) -> Inst with versions A, B, C = order."""
    verify = False
    env = {}

    def handle(self):
        enc = V.Encoder(self.p, max_frames=self.max_frames)
        if self.verify:
            enc.set_verify(True)
        return enc


# ---- encodes --------------------------------------------------------------------------------------------------------

class EncodeFrames(Case):
    """fhip_encode_subframes_dev with whole frames requested: K0 .. K4 on one stream, or (FHIP_OVERLAP=1, 512 frames
    and more) forked over aux[0..1] by ev_fork / ev_join.  Witness: oracle.encode_frame."""

    def __init__(self, oracle, nf=8, n=192, overlap=False):
        self.p, self.max_frames, self.nf, self.n, self.overlap = P(5, block_size=n), nf, nf, n, overlap
        self.env = {"FHIP_OVERLAP": "1"} if overlap else {}
        self.pcm = [signal(s, nf * n) for s in SEEDS]
        self.frames = []
        for x in self.pcm:
            fr = []
            for f in range(nf):
                rc, data, *_ = oracle.encode_frame(self.p, FIRST + f, x[f * n:(f + 1) * n], n)
                assert rc > 0
                fr.append(data)
            self.frames.append(fr)
        self.sig = [b"".join(d.tobytes() for d in fr) for fr in self.frames]

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t, nf, n = _torch, self.nf, self.n
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        stride, slot = enc.frame_stride(n), V.rice_slot_bytes(self.p, n)
        o = dict(info=Guarded(t, nf * 2 * V.INFO_DTYPE.itemsize, t.uint8, 0xA5),
                 rice=Guarded(t, nf * 2 * slot, t.uint8, 0xA5),
                 frames=Guarded(t, nf * stride, t.uint8, 0xA5),
                 frame_bytes=Guarded(t, nf, t.int32, -77))
        want = self.frames[order[1]]

        def entry(S):
            enc.encode_subframes_dev(pcm.dev, nf, n, o["info"].win, rice_bits=o["rice"].win, slot_bytes=slot,
                                     frames=o["frames"].win, frame_stride=stride, frame_bytes=o["frame_bytes"].win,
                                     first_frame_number=FIRST)
            # run_pipeline (api.hip) makes ONE run_range call for an unsplit batch and TWO, one per half on aux[0] and
            # aux[1], for a split one; each call logs K0 .. K4 once, so a split batch's list is the same names twice.
            # (A reading of the log's shape, not a flag: an unsplit list that repeated itself would read as split.)
            log = enc.last_launches()
            h = len(log) // 2
            split = len(log) >= 2 and len(log) % 2 == 0 and log[:h] == log[h:]
            assert split == self.overlap, ("the two-stream split of run_pipeline", self.overlap, log)

        def frames_ok(host):
            for f, d in enumerate(want):
                assert host[f * stride:f * stride + len(d)].tobytes() == d.tobytes(), f"frame {f} is not the oracle's"

        return Inst([pcm], o, entry, dict(frames=frames_ok, frame_bytes=eq(sizes_of(want), "frame_bytes")))


class VbsDev(Case):
    """fhip_encode_blocks_vbs_dev: the bins fanned over the aux lanes (FanJoin) and joined; with set_verify, K5 chained
    behind on the same stream.  Witness: the oracle's flake_encode_frame() loop."""

    def __init__(self, oracle, level=10, ch=2, bps=16, verify=False, nb=6, n=1024):
        from test_host_frames import oracle_stream
        self.p, self.max_frames, self.nb, self.n, self.ch, self.verify = (P(level, channels=ch, bits_per_sample=bps,
                                                                            block_size=n), 8 * nb, nb, n, ch, verify)
        self.pcm, self.exp, self.esizes, self.nfr = [], [], [], []
        for s in SEEDS:
            x = signal(s, nb * n, ch, bps).reshape(nb, n, ch).copy()
            for b in range(nb):                      # a quiet first part of 1 .. 6 eighths: the splitter cuts there
                x[b, :(1 + b) * n // 8] //= 64
            exp, esizes = oracle_stream(oracle, self.p, x.reshape(-1, ch), n)
            self.pcm.append(x)
            self.exp.append(exp)
            self.esizes.append(np.asarray(esizes, np.int32))
            self.nfr.append(np.array([max(oracle.vbs_split(x[b], ch, n)[0], 1) for b in range(nb)], np.int32))
        self.sig = [e.tobytes() for e in self.exp]

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t, nb, n = _torch, self.nb, self.n
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        cap = self.pcm[0].size * 5 + 4096
        o = dict(packed=Guarded(t, cap, t.uint8, 0xA5), totals=Guarded(t, 4, t.int64, -77),
                 frame_bytes=Guarded(t, 8 * nb, t.int32, -77), block_bytes=Guarded(t, nb, t.int32, -77),
                 block_frames=Guarded(t, nb, t.int32, -77))
        b = order[1]
        exp, nfr = self.exp[b], self.nfr[b]

        def entry(S):
            enc.encode_blocks_vbs_dev(pcm.dev, nb, n, o["packed"].win, cap, o["totals"].win,
                                      frame_bytes=o["frame_bytes"].win, block_bytes=o["block_bytes"].win,
                                      block_frames=o["block_frames"].win, first_frame_number=0)

        def totals_ok(host):
            # frames, bytes, (largest frame), flags: bit 2 would be a frame that failed K5 under set_verify
            assert (int(host[0]), int(host[1]), int(host[3])) == (int(nfr.sum()), exp.size, 0), list(host)

        return Inst([pcm], o, entry, dict(packed=prefix(exp, "packed stream"), totals=totals_ok,
                                          block_bytes=eq(self.esizes[b], "block_bytes"),
                                          block_frames=eq(nfr, "block_frames")))


# ---- verification ---------------------------------------------------------------------------------------------------

CHANGED_AT = (321, 1)            # the sample (and channel) of a frame that a "changed" version changes


def changed_signal(f):
    x = signal(SEEDS[1]).copy()
    x[f * N_DEC + CHANGED_AT[0], CHANGED_AT[1]] ^= 0x10
    return x


class Verify(Case):
    """K5's five device entries (mode: sequence = fhip_verify_frames_dev, numbered, ragged, blocks, blocks_ragged; the
    last two on an allow_vbs handle, frames numbered by sample): stream, tables and PCM are all inputs; `poison` names
    the one that the harness rewrites (the other is the good signal's).  A version is the good signal or the signal with
    ONE sample changed in one frame: the summary and the records must name exactly that frame, subframe and sample."""

    def __init__(self, oracle, mode="sequence", poison="pcm"):
        blocks = mode.startswith("blocks")
        self.mode, self.blocks, self.poison = mode, blocks, poison
        self.p = P(9, block_size=N_DEC) if blocks else P(5, block_size=N_DEC)
        self.max_frames = 96 if blocks else NF_DEC
        self.bad = [2, 5, None] if poison == "pcm" else [2, None, 9]
        good = verbatim_frames(SEEDS[1], blocks)
        self.fb = sizes_of(good)
        self.pcm, self.stream = [], []
        for f in self.bad:
            x = signal(SEEDS[1]) if f is None else changed_signal(f)
            self.pcm.append(x)
            fr = list(good)
            if f is not None:
                fr[f] = verbatim_frame(x[f * N_DEC:(f + 1) * N_DEC], f * N_DEC if blocks else f, blocks)
            assert sizes_of(fr).tolist() == self.fb.tolist()
            self.stream.append(as_u8(fr))
        self.sig = [repr(f).encode() for f in self.bad]

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        good_pcm, good_stream = signal(SEEDS[1]).reshape(-1), as_u8(verbatim_frames(SEEDS[1], self.blocks))
        if self.poison == "pcm":
            bulk = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
            d_pcm, d_stream = bulk.dev, up(good_stream)
        else:
            bulk = Bulk(t, *(self.stream[v] for v in order))
            d_pcm, d_stream = up(good_pcm), bulk.dev
        d_fb = up(self.fb)
        d_first = up((np.arange(NF_DEC) * N_DEC).astype(np.int32))           # block_first (uint32 values)
        d_num, d_sizes = up(np.arange(NF_DEC, dtype=np.int32)), up(np.full(NF_DEC, N_DEC, np.int32))
        d_src = up(np.arange(NF_DEC, dtype=np.int64) * N_DEC * 2)            # offsets in interleaved values
        d_start = up(np.arange(NF_DEC + 1, dtype=np.int64) * N_DEC)
        mode, lib = self.mode, enc.lib
        o = dict(summary=Guarded(t, 4, t.int64, 99), records=Guarded(t, NF_DEC * 4, t.int32, 99))
        nbytes, ns = int(self.fb.sum()), NF_DEC * N_DEC
        f = self.bad[order[1]]

        def entry(S):
            summ, recs = o["summary"].win, o["records"].win
            vi = V.VerifyIn(d_stream.data_ptr(), nbytes, d_fb.data_ptr(), NF_DEC, d_pcm.data_ptr(), ns, 0)
            vo = V.VerifyOut(recs.data_ptr(), summ.data_ptr())
            if mode == "sequence":
                enc.verify_frames_dev(d_stream, nbytes, d_fb, NF_DEC, d_pcm, ns, 0, summ, recs)
            elif mode == "numbered":
                enc.verify_frames_dev(d_stream, nbytes, d_fb, NF_DEC, d_pcm, ns, 0, summ, recs, frame_numbers=d_num)
            elif mode == "ragged":
                assert lib.fhip_verify_frames_ragged_dev(enc._h, C.byref(vi), d_num.data_ptr(), d_sizes.data_ptr(),
                                                         d_src.data_ptr(), C.byref(vo)) == V.OK
            elif mode == "blocks":
                enc.verify_frames_blocks_dev(d_stream, nbytes, d_fb, NF_DEC, d_pcm, ns, d_first, NF_DEC, N_DEC, summ, recs)
            else:
                assert lib.fhip_verify_frames_blocks_ragged_dev(enc._h, C.byref(vi), d_first.data_ptr(), NF_DEC,
                                                                d_start.data_ptr(), C.byref(vo)) == V.OK

        def records_ok(host):
            r = host.reshape(NF_DEC, 4)
            for k in range(NF_DEC):
                if k != f:
                    assert tuple(r[k]) == OK_REC, (k, tuple(r[k]))
            if f is not None:
                # the frame's header is 4 bytes, its number and a CRC-8; subframe c starts behind c * (8 + n * 16) bits
                hdr = 8 * (len(verbatim_frames(SEEDS[1], self.blocks)[f]) - 2) - 2 * (8 + N_DEC * 16)
                field = hdr + CHANGED_AT[1] * (8 + N_DEC * 16) + 8 + CHANGED_AT[0] * 16
                st, bit, sub, smp = (int(v) for v in r[f])
                assert (st, sub, smp) == (V.V_SAMPLES, CHANGED_AT[1], CHANGED_AT[0]), tuple(r[f])
                assert field <= bit < field + 16, (bit, field)

        summary = [NF_DEC, 0, -1, 0] if f is None else [NF_DEC, 1, f, V.V_SAMPLES]
        return Inst([bulk], o, entry, dict(summary=eq(np.array(summary, np.int64), "summary"), records=records_ok))


# ---- decoding, windows, rows ----------------------------------------------------------------------------------------

SEG_FIRST = (0, 4, 8, 12)
SEG_LEN = 4 * N_DEC
WIN_SKIP, WIN_TAKE = (100, N_DEC + 7, 0), (2000, -1, 1500)         # windows that start in the middle of a frame
ROW_LEN = 700
ROW_OF, COL_OF = (2, 0, 1), (0, 50, 60)                           # the third window is clipped by the row's end


def window_ranges():
    """[(first sample in the stream, count)] per segment."""
    out = []
    for s in range(3):
        end = SEG_LEN if WIN_TAKE[s] < 0 else min(SEG_LEN, WIN_SKIP[s] + WIN_TAKE[s])
        out.append((s * SEG_LEN + WIN_SKIP[s], end - WIN_SKIP[s]))
    return out


def rows_conv(x, fmt, bps=16):
    return x.astype(np.float32) * np.float32(2.0 ** -(bps - 1)) if fmt == V.ROWS_F32 else x.astype(np.int32)


def rows_of(pcm, starts, counts, fmt):
    """include/flakehip.h's delivery rule in numpy, on zeroed rows [3][2][ROW_LEN]."""
    rows = np.zeros((3, 2, ROW_LEN), np.float32 if fmt == V.ROWS_F32 else np.int32)
    for k in range(3):
        m = min(counts[k], ROW_LEN - COL_OF[k])
        rows[ROW_OF[k], :, COL_OF[k]:COL_OF[k] + m] = rows_conv(pcm[starts[k]:starts[k] + m], fmt).T
    return rows


class Decode(Case):
    """fhip_decode_frames_dev / _segments_dev / _windows_dev (K7 through the handle's d_smp, d_vws, d_dclip), and
    mode "rows": windows -> fhip_rows_zero_dev -> fhip_rows_from_segments_dev chained with nothing in between, K10
    reading seg_start / seg_samples / seg_failed where K7 left them.  Witness: the source PCM, placed by numpy."""

    def __init__(self, oracle, mode="frames", fmt=V.ROWS_I32):
        self.mode, self.fmt = mode, fmt
        self.p, self.max_frames = P(5, block_size=N_DEC), NF_DEC
        self.stream = [as_u8(verbatim_frames(s)) for s in SEEDS]
        self.fb = sizes_of(verbatim_frames(SEEDS[0]))
        assert all(sizes_of(verbatim_frames(s)).tolist() == self.fb.tolist() for s in SEEDS)
        self.src = [signal(s) for s in SEEDS]
        self.sig = [self.want_pcm(v).tobytes() for v in range(3)]

    def want_pcm(self, v):
        if self.mode in ("frames", "segments"):
            return self.src[v]
        return np.concatenate([self.src[v][a:a + n] for a, n in window_ranges()])

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t, mode = _torch, self.mode
        stream = Bulk(t, *(self.stream[v] for v in order))
        d_fb = up(self.fb)
        want = self.want_pcm(order[1])
        cap = len(want)
        o = dict(pcm=Guarded(t, cap * 2, t.int32, -1234567), summary=Guarded(t, 4, t.int64, 99),
                 nsamples=Guarded(t, 1, t.int64, 99), records=Guarded(t, NF_DEC * 4, t.int32, 99))
        exp = dict(pcm=eq(want, "pcm"), summary=eq(np.array([NF_DEC, 0, -1, 0], np.int64), "summary"),
                   nsamples=eq(np.array([cap], np.int64), "nsamples"),
                   records=eq(np.tile(np.array(OK_REC, np.int32), NF_DEC), "records"))
        nbytes = int(self.fb.sum())
        if mode != "frames":
            o.update(seg_start=Guarded(t, 3, t.int64, -7), seg_samples=Guarded(t, 3, t.int64, -7),
                     seg_failed=Guarded(t, 3, t.int32, -7))
            counts = [SEG_LEN] * 3 if mode == "segments" else [n for _, n in window_ranges()]
            starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
            exp.update(seg_start=eq(starts.astype(np.int64), "seg_start"),
                       seg_samples=eq(np.array(counts, np.int64), "seg_samples"),
                       seg_failed=eq(np.full(3, -1, np.int32), "seg_failed"))
            sf, num, var = up(SEG_FIRST, np.int32), up([0, 4, 8], np.int64), up([0, 0, 0], np.int32)
            skip, take = up(WIN_SKIP, np.int64), up(WIN_TAKE, np.int64)
            seg = (sf, 3, num, var, o["seg_start"].win, o["seg_samples"].win, o["seg_failed"].win)
        if mode == "rows":
            dt = t.float32 if self.fmt == V.ROWS_F32 else t.int32
            o["rows"] = Guarded(t, 3 * 2 * ROW_LEN, dt, 12345.5 if self.fmt == V.ROWS_F32 else -1234567)
            exp["rows"] = eq(rows_of(want, starts, counts, self.fmt), "rows")
            row, col = up(ROW_OF, np.int32), up(COL_OF, np.int64)

        def entry(S):
            head = (stream.dev, nbytes, d_fb, NF_DEC, o["pcm"].win, cap, o["summary"].win, o["nsamples"].win)
            if mode == "frames":
                enc.decode_frames_dev(*head, o["records"].win, False, 0)
            elif mode == "segments":
                enc.decode_frames_segments_dev(*head, *seg, o["records"].win)
            else:
                assert enc.decode_frames_windows_dev(*head, *seg, skip, take, o["records"].win) == V.OK
            if mode == "rows":
                assert enc.rows_zero_dev(o["rows"].win, 3, ROW_LEN, self.fmt, 0, 3) == V.OK
                assert enc.rows_from_segments_dev(o["pcm"].win, cap, 3, o["seg_start"].win, o["seg_samples"].win,
                                                  o["seg_failed"].win, row, col, o["rows"].win, 3, ROW_LEN,
                                                  self.fmt) == V.OK

        return Inst([stream], o, entry, exp)


class Rows(Case):
    """fhip_rows_zero_dev + fhip_rows_from_segments_dev alone: the PCM is the input, K7's tables are fixed."""

    def __init__(self, oracle, fmt=V.ROWS_I32):
        self.fmt, self.p, self.max_frames = fmt, P(5, block_size=192), 4
        self.starts, self.counts = [0, 700, 1000], [700, 300, 650]
        self.pcm = [signal(s, 1700) for s in SEEDS]
        self.sig = [rows_of(x, self.starts, self.counts, fmt).tobytes() for x in self.pcm]

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t, fmt = _torch, self.fmt
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        dt = t.float32 if fmt == V.ROWS_F32 else t.int32
        o = dict(rows=Guarded(t, 3 * 2 * ROW_LEN, dt, 12345.5 if fmt == V.ROWS_F32 else -1234567))
        st, cn, fl = up(self.starts, np.int64), up(self.counts, np.int64), up([-1, -1, -1], np.int32)
        row, col = up(ROW_OF, np.int32), up(COL_OF, np.int64)

        def entry(S):
            assert enc.rows_zero_dev(o["rows"].win, 3, ROW_LEN, fmt, 0, 3) == V.OK
            assert enc.rows_from_segments_dev(pcm.dev, 1700, 3, st, cn, fl, row, col, o["rows"].win, 3, ROW_LEN,
                                              fmt) == V.OK

        return Inst([pcm], o, entry, dict(rows=eq(rows_of(self.pcm[order[1]], self.starts, self.counts, fmt), "rows")))


# ---- index, gather, MD5 ---------------------------------------------------------------------------------------------

INDEX_CAP = 16


class Index(Case):
    """fhip_index_frames_dev over the 12-frame stream as two ranges of six frames.  The frame table is flacgen's; a
    version is the stream itself or the stream with the CRC-16 of one frame broken, where the walk of that range stops
    (the frame is not consumed, and no later boundary closes it: the CRC-16 runs on over the broken one)."""

    def __init__(self, oracle):
        self.p, self.max_frames = P(5, block_size=N_DEC), NF_DEC
        frames = verbatim_frames(SEEDS[1])
        self.fb = sizes_of(frames)
        self.bad = [2, None, 9]
        self.stream = []
        for f in self.bad:
            s = as_u8(frames)
            if f is not None:
                s[int(self.fb[:f + 1].sum()) - 1] ^= 0x01
            self.stream.append(s)
        self.range_first = np.array([0, self.fb[:6].sum(), self.fb.sum()], np.int64)
        self.sig = [b"".join(a.tobytes() for a in self.want(v)) for v in range(3)]

    def want(self, v):
        """(frame_bytes [INDEX_CAP] with -77 behind the last frame, range_frames, range_consumed, range_variable)"""
        f = self.bad[v]
        found = [6 if f is None or f >= 6 else f, 6 if f is None or f < 6 else f - 6]
        sizes = np.concatenate([self.fb[:found[0]], self.fb[6:6 + found[1]]])
        fbytes = np.full(INDEX_CAP, -77, np.int32)
        fbytes[:len(sizes)] = sizes
        cons = np.array([self.fb[:found[0]].sum(), self.fb[6:6 + found[1]].sum()], np.int64)
        return fbytes, np.array(found, np.int32), cons, np.zeros(2, np.int32)

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        stream = Bulk(t, *(self.stream[v] for v in order))
        rf = up(self.range_first)
        o = dict(frame_bytes=Guarded(t, INDEX_CAP, t.int32, -77), range_frames=Guarded(t, 2, t.int32, -77),
                 range_consumed=Guarded(t, 2, t.int64, -77), range_variable=Guarded(t, 2, t.int32, -77))
        nbytes = int(self.fb.sum())

        def entry(S):
            enc.index_ranges_dev(stream.dev, nbytes, rf, 2, N_DEC, INDEX_CAP, o["frame_bytes"].win,
                                 o["range_frames"].win, o["range_consumed"].win, o["range_variable"].win)

        w = self.want(order[1])
        return Inst([stream], o, entry, {k: eq(a, k) for k, a in zip(o, w)})


# (src_buf, src, dst, count); the second table is what the second call of the back-to-back sequence brings, so that a
# host image rewritten under a pending copy would show
GATHER_ROWS = ([(0, 5, 0, 700), (1, 3, 700, 100), (0, 1200, 800, 1), (1, 600, 801, 333), (0, 64, 1134, 250)],
               [(1, 700, 0, 250), (0, 9, 250, 333), (1, 2, 583, 1), (0, 1100, 584, 700), (1, 1400, 1284, 100)])
GATHER_TOTAL, GATHER_CAPS = 1384, (2000, 1500)


class Gather(Case):
    """fhip_gather_spans_dev: five pieces from two sources, one (700 stereo samples) longer than a K9 tile of 1024
    values; the piece table goes through the handle's host image h_gather.  Witness: numpy."""

    def __init__(self, oracle):
        self.p, self.max_frames = P(5, block_size=192), 4
        r = np.random.RandomState(9)
        self.src = [[r.randint(-2 ** 31, 2 ** 31 - 1, size=(c, 2), dtype=np.int64).astype(np.int32) for c in GATHER_CAPS]
                    for _ in SEEDS]
        self.sig = [self.want(v).tobytes() for v in range(3)]
        assert all(sum(r[3] for r in rows) == GATHER_TOTAL for rows in GATHER_ROWS)

    def want(self, v, variant=0):
        out = np.zeros((GATHER_TOTAL, 2), np.int32)
        for buf, src, dst, count in GATHER_ROWS[variant]:
            out[dst:dst + count] = self.src[v][buf][src:src + count]
        return out

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        s0, s1 = (Bulk(t, *(self.src[v][k].reshape(-1) for v in order)) for k in (0, 1))
        o = dict(dst=Guarded(t, GATHER_TOTAL * 2, t.int32, -1234567))
        pieces = V.gather_pieces(GATHER_ROWS[variant])

        def entry(S):
            assert enc.gather_spans_dev(o["dst"].win, GATHER_TOTAL, s0.dev, GATHER_CAPS[0], s1.dev, GATHER_CAPS[1],
                                        pieces) == V.OK

        return Inst([s0, s1], o, entry, dict(dst=eq(self.want(order[1], variant), "dst")))


def md5_message(vals, bits=16):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(vals.astype("<i4")).reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


MD5_N, MD5_NB, MD5_S = 192, 8, 3
MD5_UPDATES = (([0, 2, 3, 5], [0, 3, 1, 2, 4]), ([0, 1, 1, 3], [5, 6, 7]))       # (seg_first, seg_block) per update
MD5_RANGES = dict(seg_first=[0, 1, 2, 2], seg_range=[1, 0], start=[10, 500], samples=[100, 333])


class Md5Chain(Case):
    """fhip_md5_init_dev -> _update_dev x 2 -> _update_ranges_dev -> _final_dev, one chain with nothing in between; the
    digests are the output.  Witness: hashlib over the PCM packed at (bits + 7) / 8 bytes."""

    def __init__(self, oracle):
        self.p, self.max_frames = P(5, block_size=MD5_N), MD5_NB
        self.pcm = [signal(s, MD5_NB * MD5_N) for s in SEEDS]
        self.sig = [self.want(v).tobytes() for v in range(3)]

    def want(self, v):
        x = self.pcm[v]
        h = [hashlib.md5() for _ in range(MD5_S)]
        for first, block in MD5_UPDATES:
            for s in range(MD5_S):
                for b in block[first[s]:first[s + 1]]:
                    h[s].update(md5_message(x[b * MD5_N:(b + 1) * MD5_N]))
        r = MD5_RANGES
        for s in range(MD5_S):
            for k in r["seg_range"][r["seg_first"][s]:r["seg_first"][s + 1]]:
                h[s].update(md5_message(x[r["start"][k]:r["start"][k] + r["samples"][k]]))
        return np.frombuffer(b"".join(m.digest() for m in h), np.uint8)

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        o = dict(states=Guarded(t, MD5_S * V.MD5_STATE_BYTES, t.uint8, 0xA5), digests=Guarded(t, MD5_S * 16, t.uint8, 0xA5))
        tabs = [(up(f, np.int32), up(b, np.int32)) for f, b in MD5_UPDATES]
        r = MD5_RANGES
        rt = (up(r["seg_first"], np.int32), up(r["seg_range"], np.int32), up(r["start"], np.int64),
              up(r["samples"], np.int64))

        def entry(S):
            st = o["states"].win
            enc.md5_init_dev(st, MD5_S)
            for f, b in tabs:
                enc.md5_update_dev(st, MD5_S, pcm.dev, MD5_N, f, b)
            enc.md5_update_ranges_dev(st, MD5_S, pcm.dev, *rt)
            enc.md5_final_dev(st, MD5_S, o["digests"].win)

        return Inst([pcm], o, entry, dict(digests=eq(self.want(order[1]), "digests")))


MD5_PREFIX = 100                 # samples behind a state input: 400 bytes, so 16 wait in its tail


class Md5StatesInput(Case):
    """The running states as a poisoned INPUT: fhip_md5_update_dev then fhip_md5_final_dev on states that the caller's
    stream brings.  A, B and C are valid states -- fhip_md5_init_dev plus one update of MD5_PREFIX samples of three
    different signals, made on the device when the case is prepared and copied to the host -- so an update or a final
    that read the buffer too early or too late hashes behind another prefix.  The PCM of the update under test is the
    same in every version.  Witness: hashlib over prefix + block."""

    def __init__(self, oracle):
        self.p, self.max_frames = P(5, block_size=MD5_N), MD5_S
        self.prefix = [signal(s + 1, MD5_S * MD5_PREFIX) for s in SEEDS]
        self.block = signal(505, MD5_S * MD5_N)
        self.sig = [self.want(v).tobytes() for v in range(3)]

    def want(self, v):
        out = b""
        for s in range(MD5_S):
            out += hashlib.md5(md5_message(self.prefix[v][s * MD5_PREFIX:(s + 1) * MD5_PREFIX]) +
                               md5_message(self.block[s * MD5_N:(s + 1) * MD5_N])).digest()
        return np.frombuffer(out, np.uint8)

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        first, block = up(np.arange(MD5_S + 1, dtype=np.int32)), up(np.arange(MD5_S, dtype=np.int32))
        made = []
        for v in order:                              # the three state versions, synchronously, before the harness starts
            tmp = t.zeros(MD5_S * V.MD5_STATE_BYTES, dtype=t.uint8, device="cuda")
            d_prefix = up(self.prefix[v].reshape(-1))
            t.cuda.synchronize()
            enc.md5_init_dev(tmp, MD5_S)
            enc.md5_update_dev(tmp, MD5_S, d_prefix, MD5_PREFIX, first, block)
            enc.sync()
            made.append(tmp.cpu().numpy())
        fill = np.frombuffer(made[0].tobytes(), V.MD5_STATE_DTYPE)["fill"]
        assert (fill == (MD5_PREFIX * 2 * 2) % 64).all() and not any(np.array_equal(made[i], made[j])
                                                                       for i, j in ((0, 1), (0, 2), (1, 2)))
        states = Bulk(t, *made)
        d_pcm = up(self.block.reshape(-1))
        o = dict(digests=Guarded(t, MD5_S * 16, t.uint8, 0xA5))

        def entry(S):
            enc.md5_update_dev(states.dev, MD5_S, d_pcm, MD5_N, first, block)
            enc.md5_final_dev(states.dev, MD5_S, o["digests"].win)

        return Inst([states], o, entry, dict(digests=eq(self.want(order[1]), "digests")))


class Md5AcrossStreams(Case):
    """fhip_frames_packed_upload + fhip_md5_update_uploaded (on the handle's md5_stream) and fhip_md5_update_dev (on the
    caller's stream) on the SAME states, in either order, then fhip_md5_final_dev: the digest is hashlib's over both
    blocks in call order (the comment above md5_dev_begin in api.hip).  The uploaded blocks are host memory and the
    same in every version; the device blocks are the poisoned input.

    fhip_frames_packed_upload(_ragged) synchronises the handle's stream before it returns (api.hip, the
    hipStreamSynchronize behind stage_pcm), so in all of these cases the gate has opened, and B has landed, before the
    hand-over between md5_stream and the caller's stream is queued: the two events are exercised at natural timing
    only, with poison C queued behind the final.  That follows from the entry; the log shows it as "returned after the
    gate had opened"."""

    def __init__(self, oracle, uploaded_first=True, ragged=False):
        self.uploaded_first, self.ragged = uploaded_first, ragged
        self.p, self.max_frames = P(5, block_size=MD5_N), MD5_S
        # the uploaded blocks: MD5_S of MD5_N samples, or (fhip_frames_packed_upload_ragged) of their own lengths
        self.sizes = np.array([MD5_N, 100, 51] if ragged else [MD5_N] * MD5_S, np.int32)
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)])
        self.host_pcm = np.ascontiguousarray(signal(404, int(self.sizes.sum())))
        self.pcm = [signal(s, MD5_S * MD5_N) for s in SEEDS]
        self.sig = [self.want(v).tobytes() for v in range(3)]

    BLOCK_OF = ((0, 1, 2), (1, 2, 0))          # the uploaded block stream s absorbs, per variant (the second call's differs)

    def want(self, v, variant=0):
        out = b""
        for s in range(MD5_S):
            u = self.BLOCK_OF[variant][s]
            parts = [md5_message(self.host_pcm[self.starts[u]:self.starts[u + 1]]),
                     md5_message(self.pcm[v][s * MD5_N:(s + 1) * MD5_N])]
            out += hashlib.md5(b"".join(parts if self.uploaded_first else parts[::-1])).digest()
        return np.frombuffer(out, np.uint8)

    def instance(self, enc, order=(0, 1, 2), variant=0):
        t = _torch
        pcm = Bulk(t, *(self.pcm[v].reshape(-1) for v in order))
        o = dict(states=Guarded(t, MD5_S * V.MD5_STATE_BYTES, t.uint8, 0xA5), digests=Guarded(t, MD5_S * 16, t.uint8, 0xA5))
        first, block = np.arange(MD5_S + 1, dtype=np.int32), np.array(self.BLOCK_OF[variant], np.int32)
        d_first, d_block = up(first), up(np.arange(MD5_S, dtype=np.int32))
        lib, host = enc.lib, self.host_pcm
        batch = V.Batch(pcm=host.ctypes.data, nframes=MD5_S, block_size=MD5_N)

        sizes = self.sizes

        def uploaded(st):
            if self.ragged:
                assert lib.fhip_frames_packed_upload_ragged(enc._h, C.byref(batch), sizes.ctypes.data) == V.OK
                assert lib.fhip_md5_update_uploaded_ragged(enc._h, V._ptr(st), MD5_S, MD5_S, sizes.ctypes.data,
                                                           first.ctypes.data, block.ctypes.data) == V.OK
                return
            assert lib.fhip_frames_packed_upload(enc._h, C.byref(batch)) == V.OK
            assert lib.fhip_md5_update_uploaded(enc._h, V._ptr(st), MD5_S, MD5_S, MD5_N, first.ctypes.data,
                                                block.ctypes.data) == V.OK

        def entry(S):
            st = o["states"].win
            enc.md5_init_dev(st, MD5_S)
            if self.uploaded_first:
                uploaded(st)
            enc.md5_update_dev(st, MD5_S, pcm.dev, MD5_N, d_first, d_block)
            if not self.uploaded_first:
                uploaded(st)
            enc.md5_final_dev(st, MD5_S, o["digests"].win)

        return Inst([pcm], o, entry, dict(digests=eq(self.want(order[1], variant), "digests")))


# ---- the case table -------------------------------------------------------------------------------------------------

class Spec:
    def __init__(self, id, entries, factory, **kw):
        self.id, self.entries, self.factory, self.kw = id, tuple(entries), factory, kw

    def build(self, oracle):
        return self.factory(oracle, **self.kw)


CASES = [
    Spec("encode_frames", ["fhip_encode_subframes_dev"], EncodeFrames),
    Spec("encode_frames_overlap", ["fhip_encode_subframes_dev"], EncodeFrames, nf=512, overlap=True),
    Spec("vbs_level10_stereo16", ["fhip_encode_blocks_vbs_dev"], VbsDev, level=10),
    Spec("vbs_level12_stereo16", ["fhip_encode_blocks_vbs_dev"], VbsDev, level=12),
    Spec("vbs_level10_3ch24", ["fhip_encode_blocks_vbs_dev"], VbsDev, level=10, ch=3, bps=24),
    Spec("vbs_level12_3ch24", ["fhip_encode_blocks_vbs_dev"], VbsDev, level=12, ch=3, bps=24),
    Spec("vbs_level10_verify", ["fhip_encode_blocks_vbs_dev"], VbsDev, level=10, verify=True),
    Spec("verify_pcm", ["fhip_verify_frames_dev"], Verify, poison="pcm"),
    Spec("verify_stream", ["fhip_verify_frames_dev"], Verify, poison="stream"),
    Spec("verify_numbered_pcm", ["fhip_verify_frames_numbered_dev"], Verify, mode="numbered", poison="pcm"),
    Spec("verify_ragged_stream", ["fhip_verify_frames_ragged_dev"], Verify, mode="ragged", poison="stream"),
    Spec("verify_blocks_pcm", ["fhip_verify_frames_blocks_dev"], Verify, mode="blocks", poison="pcm"),
    Spec("verify_blocks_stream", ["fhip_verify_frames_blocks_dev"], Verify, mode="blocks", poison="stream"),
    Spec("verify_blocks_ragged_pcm", ["fhip_verify_frames_blocks_ragged_dev"], Verify, mode="blocks_ragged", poison="pcm"),
    Spec("decode_frames", ["fhip_decode_frames_dev"], Decode, mode="frames"),
    Spec("decode_segments", ["fhip_decode_frames_segments_dev"], Decode, mode="segments"),
    Spec("decode_windows", ["fhip_decode_frames_windows_dev"], Decode, mode="windows"),
    Spec("rows_i32", ["fhip_rows_from_segments_dev", "fhip_rows_zero_dev"], Rows, fmt=V.ROWS_I32),
    Spec("rows_f32", ["fhip_rows_from_segments_dev", "fhip_rows_zero_dev"], Rows, fmt=V.ROWS_F32),
    Spec("decode_then_rows_i32", ["fhip_decode_frames_windows_dev", "fhip_rows_zero_dev", "fhip_rows_from_segments_dev"],
         Decode, mode="rows", fmt=V.ROWS_I32),
    Spec("decode_then_rows_f32", ["fhip_decode_frames_windows_dev", "fhip_rows_zero_dev", "fhip_rows_from_segments_dev"],
         Decode, mode="rows", fmt=V.ROWS_F32),
    Spec("index_ranges", ["fhip_index_frames_dev"], Index),
    Spec("gather_spans", ["fhip_gather_spans_dev"], Gather),
    Spec("md5_chain", ["fhip_md5_init_dev", "fhip_md5_update_dev", "fhip_md5_update_ranges_dev", "fhip_md5_final_dev"],
         Md5Chain),
    Spec("md5_states_as_input", ["fhip_md5_init_dev", "fhip_md5_update_dev", "fhip_md5_final_dev"], Md5StatesInput),
    Spec("md5_uploaded_then_dev", ["fhip_md5_update_uploaded", "fhip_md5_update_dev", "fhip_md5_final_dev"],
         Md5AcrossStreams, uploaded_first=True),
    Spec("md5_dev_then_uploaded", ["fhip_md5_update_uploaded", "fhip_md5_update_dev", "fhip_md5_final_dev"],
         Md5AcrossStreams, uploaded_first=False),
    Spec("md5_uploaded_ragged_then_dev", ["fhip_md5_update_uploaded_ragged", "fhip_md5_update_dev", "fhip_md5_final_dev"],
         Md5AcrossStreams, uploaded_first=True, ragged=True),
]
# entries whose ordering tests are sequences of their own below, not rows of the table
SEQUENCE_ENTRIES = {"fhip_frames_packed_fetch_async": "test_fetch_overlap"}

_BUILT = {}


def built(spec, oracle):
    """The CPU side of a case, made once per session and never changed."""
    if spec.id not in _BUILT:
        _BUILT[spec.id] = spec.build(oracle)
    return _BUILT[spec.id]


def ordered(enc, name, insts):
    """One pass through the harness for one or more prepared calls on one handle, queued back to back."""
    _torch.cuda.synchronize()
    outputs = {f"{k}.{name_}": g for k, i in enumerate(insts) for name_, g in i.outputs.items()}
    expected = {f"{k}.{name_}": e for k, i in enumerate(insts) for name_, e in i.expected.items()}

    def entry(S):
        for i in insts:
            i.entry(S)

    return SO.run_ordered(_torch, name, entry, [b for i in insts for b in i.inputs], outputs, expected, enc.set_stream)


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_entry_is_ordered_on_its_stream(control, oracle, monkeypatch, spec):
    case = built(spec, oracle)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)                        # (fhip_create reads it)
    with case.handle() as enc:
        ordered(enc, spec.id, [case.instance(enc)]).assert_clean()


@pytest.mark.parametrize("spec", CASES, ids=lambda s: s.id)
def test_back_to_back(control, oracle, monkeypatch, spec):
    """The entry twice in a row, on inputs B1 then B2 into separate outputs, behind one gate: the second call rewrites
    the handle's host images and workspaces while the first may still be pending.  Both must be right.  Where an entry
    takes a host table (the gather's pieces, the uploaded MD5's segments), the second call brings a different one."""
    case = built(spec, oracle)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    with case.handle() as enc:
        calls = [case.instance(enc, (0, 1, 2)), case.instance(enc, (1, 2, 0), variant=1)]
        ordered(enc, spec.id + " twice", calls).assert_clean()


# ---- sequences ------------------------------------------------------------------------------------------------------

def test_switching_streams(control, oracle):
    """The gate closed on S1 and an encode called there; then, from the caller's side, S2.wait_stream(S1) and
    set_stream(S2), and a decode -- which passes through the encoder's sample workspace -- on S2.  fhip_set_stream only
    swaps a pointer: the order between the two streams is the caller's.  Both results must be right; afterwards
    set_stream(None) behind enc.sync() behaves as before."""
    e_case = EncodeFrames(oracle, nf=NF_DEC, n=N_DEC)
    d_case = built(next(s for s in CASES if s.id == "decode_frames"), oracle)
    with V.Encoder(P(5, block_size=N_DEC), max_frames=NF_DEC) as enc:
        e, d = e_case.instance(enc), d_case.instance(enc)
        S2 = _torch.cuda.Stream()
        _torch.cuda.synchronize()
        outputs = {**{"enc." + k: g for k, g in e.outputs.items()}, **{"dec." + k: g for k, g in d.outputs.items()}}
        expected = {**{"enc." + k: g for k, g in e.expected.items()}, **{"dec." + k: g for k, g in d.expected.items()}}

        def entry(S1):
            enc.set_stream(S1.cuda_stream)
            e.entry(S1)
            S2.wait_stream(S1)                       # (the decode's input was copied in on S1 as well)
            enc.set_stream(S2.cuda_stream)
            with _torch.cuda.stream(S2):
                d.entry(S2)
            S1.wait_stream(S2)                       # the harness looks at everything from S1

        SO.run_ordered(_torch, "switching streams (encode on S1, decode on S2)", entry, e.inputs + d.inputs, outputs,
                       expected, enc.set_stream).assert_clean()
        # back on the handle's own stream: a synchronous encode gives the oracle's frames as before
        enc.sync()
        enc.set_stream(None)
        pcm = _torch.from_numpy(e_case.pcm[1].reshape(-1).copy()).cuda()
        for g in e.outputs.values():
            g.fill()
        _torch.cuda.synchronize()
        e.inputs[0].dev.copy_(pcm)
        _torch.cuda.synchronize()
        e.entry(None)
        enc.sync()
        for k, chk in e.expected.items():
            chk(e.outputs[k].win.cpu().numpy())


@pytest.mark.parametrize("second", ["frames_packed_begin", "encode_blocks_vbs_packed_numbered"])
def test_fetch_overlap(control, oracle, second):
    """fhip_frames_packed_begin for batch 1, fhip_frames_packed_fetch_async into pinned memory, the next encode at once,
    then fetch_wait: the download reads d_packed on aux[0] while the second call is about to overwrite it, and the
    second call must wait for ev_fetch.  The first fetch must hold batch 1's bytes exactly, as oracle.encode_frame
    gives them.  With encode_blocks_vbs_packed_numbered as the second call the wait is the
    `block_first && c->fetch_pending` branch of the variable-block-size path.

    What this sequence checks is the RESULT, not the race: fhip_frames_packed_begin synchronises the handle's stream
    before it returns, so the gate (queued on that stream before the first call, with an event behind it that is queried
    when the first call returns) only delays it, and a download of six small frames on aux[0] is over long before the
    second call reaches d_packed.  A missing ev_fetch wait would most likely still pass here."""
    vbs = second != "frames_packed_begin"
    n, nf = 1024, 6
    p = P(10, block_size=n) if vbs else P(5, block_size=n)
    step = n if vbs else 1                                         # allow_vbs: frames are numbered by sample
    pcm1, pcm2 = (np.ascontiguousarray(signal(s, nf * n)) for s in SEEDS[:2])
    want1 = [oracle.encode_frame(p, f * step, pcm1[f * n:(f + 1) * n], n)[1] for f in range(nf)]
    lib = V.load_library()
    with V.Encoder(p, max_frames=8 * nf) as enc:
        cap = nf * enc.frame_stride(n) + 64
        out1 = _torch.full((cap,), 0xA5, dtype=_torch.uint8).pin_memory()
        fb1, fb2 = np.zeros(nf, np.int32), np.zeros(nf, np.int32)
        b1 = V.Batch(pcm=pcm1.ctypes.data, nframes=nf, block_size=n, frame_bytes=fb1.ctypes.data)
        b2 = V.Batch(pcm=pcm2.ctypes.data, nframes=nf, block_size=n, frame_bytes=fb2.ctypes.data)
        total = C.c_int64(0)
        t_e = gate_ms = 0.0
        early = None
        for warm in (True, False):
            S = _torch.cuda.Stream()
            enc.set_stream(S.cuda_stream)
            e_gate = None
            if not warm:
                out1.fill_(0xA5)
                gate_ms = SO.gate_ms_for(t_e)
                with _torch.cuda.stream(S):
                    SO.queue_gate(_torch, gate_ms)
                    e_gate = _torch.cuda.Event()
                    e_gate.record(S)
                    assert not e_gate.query(), "harness: the gate was open before the first call"
            t0 = time.perf_counter()
            assert lib.fhip_frames_packed_begin(enc._h, C.byref(b1), C.byref(total)) == V.OK
            if e_gate is not None:
                early = not e_gate.query()                         # the observation: noted, not asserted
            total1 = total.value
            # (the shared library object has no argtypes for the next two entries: the values are wrapped here)
            assert lib.fhip_frames_packed_fetch_async(enc._h, C.c_void_p(out1.data_ptr()), C.c_int64(cap)) == V.OK
            if vbs:
                got2 = enc.encode_blocks_vbs_packed_numbered(pcm2, n, np.arange(nf, dtype=np.uint32) * n)
            else:
                assert lib.fhip_frames_packed_begin(enc._h, C.byref(b2), C.byref(total)) == V.OK
            assert lib.fhip_frames_packed_fetch_wait(enc._h) == V.OK
            if warm:
                t_e = (time.perf_counter() - t0) * 1e3             # the whole sequence, warm and synchronous
            got1 = out1.numpy()
            assert fb1.tolist() == [len(d) for d in want1] and total1 == int(fb1.sum())
            assert got1[:total1].tobytes() == b"".join(d.tobytes() for d in want1), "the first fetch is not batch 1"
            assert (got1[total1:] == 0xA5).all()
            # the second batch is right as well
            if vbs:
                from test_host_frames import oracle_stream
                exp2, _ = oracle_stream(oracle, p, pcm2, n)
                assert got2[0].tobytes() == exp2.tobytes()
            else:
                out2 = np.zeros(cap, np.uint8)
                assert lib.fhip_frames_packed_fetch(enc._h, out2.ctypes.data, cap) == V.OK
                want2 = b"".join(oracle.encode_frame(p, f, pcm2[f * n:(f + 1) * n], n)[1].tobytes() for f in range(nf))
                assert out2[:total.value].tobytes() == want2
            enc.sync()
            enc.set_stream(None)
    SO.log_observation(f"fetch overlap ({second} second), first fhip_frames_packed_begin", t_e, gate_ms, early)


def test_decode_set_rows_into_a_tensor_with_work_pending(control):
    """The Python layer: DecodeSet.decode_windows_rows(out=t) under torch.cuda.stream(S) with the gate closed on S and a
    garbage fill of t queued behind the gate.  The set's handle runs on a stream of its own, and the method drains
    torch's current stream by hand before the call: after the call and S.synchronize(), t must hold the windows (numpy
    over the source PCM), and the garbage fill must not land afterwards."""
    t = _torch
    frames = verbatim_frames(SEEDS[1])
    fb, src = sizes_of(frames), signal(SEEDS[1])
    off = np.concatenate([[0], np.cumsum(fb)])
    stream = as_u8(frames)
    like = V.HostStreaminfo(min_block_size=N_DEC, max_block_size=N_DEC, sample_rate=44100, channels=2, bits_per_sample=16)
    # (run bytes, frame sizes, fixed block size, first sample, count): from the stream's start, and from frame 7 on
    wins = [(stream, fb, N_DEC, 1000, ROW_LEN), (stream[off[7]:], fb[7:], N_DEC, 7 * N_DEC + 333, 500),
            (stream[off[3]:], fb[3:], N_DEC, 3 * N_DEC, 650)]
    want = np.zeros((3, 2, ROW_LEN), np.float32)
    for w, (_, _, _, first, count) in enumerate(wins):
        m = min(count, ROW_LEN)
        want[w, :, :m] = rows_conv(src[first:first + m], V.ROWS_F32).T
    with V.DecodeSet(like, 1, V.SET_MD5_OFF) as g:
        g.decode_windows_rows(wins, ROW_LEN)                       # (nothing lazy under the gate)
        t0 = time.perf_counter()
        g.decode_windows_rows(wins, ROW_LEN)                       # warm and synchronous: T_e
        t_e = (time.perf_counter() - t0) * 1e3
        gate_ms = SO.gate_ms_for(t_e)
        out = t.zeros((3, 2, ROW_LEN), dtype=t.float32, device="cuda")
        t.cuda.synchronize()
        S = t.cuda.Stream()
        with t.cuda.stream(S):
            SO.queue_gate(t, gate_ms)
            e_gate = t.cuda.Event()
            e_gate.record(S)
            assert not e_gate.query(), "harness: the gate was open before the call"
            out.fill_(12345.5)                                     # the garbage, behind the gate
            rows, lengths, status, _ = g.decode_windows_rows(wins, ROW_LEN, out=out)
            early = not e_gate.query()                             # the observation: noted, not asserted
            snap = rows.clone()
            S.synchronize()
        assert lengths.tolist() == [ROW_LEN, 500, 650] and list(status) == [0, 0, 0]
        assert np.array_equal(snap.cpu().numpy(), want)
        t.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), "something landed after the call"
    SO.log_observation("DecodeSet.decode_windows_rows(out=)", t_e, gate_ms, early)
