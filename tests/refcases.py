"""The case table of the reference witness, and the tools around its record files.  TEST INFRASTRUCTURE ONLY.

oracle/ref_frames.c is one libflake client built twice (oracle/Makefile, `refframes`): oracle/_ref/build/ref_frames on
the reference's own static library (the witness) and oracle/_ref/ref_frames_hip on this project's libflake.so (the
subject).  Every case below is one run of that client: a format, a compression level, overrides of FlakeEncodeParams
members and a PCM signal.  tests/test_ref_witness_cpu.py holds oracle/flake_oracle.c to the witness over the whole
table, tests/test_gpu_ref_witness.py holds the HIP frames to the witness's record (tests/golden/ref_frames.npz, made
by tests/golden/make_golden.py) over every case that is not of the `random` family.

Signals come from integer arithmetic alone (Generator.integers, a parabolic integer sine, shifts, clips): the same PCM
on every machine, and the record keeps its SHA-1, so that a drift in generation shows as a drift.

A case is ADMISSIBLE only if every frame it can produce is defined in the reference (admissible() below; the table is
held to it by a test, nothing is skipped at run time):
  * under FLAKE_PREDICTION_LEVINSON every frame -- each block, the tail, each run of eighths a variable-block-size
    split can cut a block into -- has even length (lpc.c:35,53 leaves the window's centre element uninitialised for odd
    lengths) and, when max_prediction_order > 4, is longer than max_prediction_order (optimize.c:168-173 then indexes
    bits[5] with min_prediction_order);
  * no 32-bit case has two channels with stereo_method 1: the side channel is 33 bits wide and
    bitwriter_writebits(33, ..) shifts a 32-bit value by 33 (bitio.h:103);
  * a 32-bit case's signal stays within 28 bits (Case.signal_bits).  bitwriter_write_rice_signed computes -2*val-1 in
    an int (bitio.h:128), which overflows for a residual of 2^30 and more, and the frame then no longer decodes to its
    input: format_1ch_32bit_level9 on a full-scale transient lost 128 samples that way, oracle and witness byte for
    byte alike.  16 times below full scale no residual an order search tries gets there, and every case is held to
    the round trip through oracle/flac_decode.c, which would show it.
"""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
WITNESS = os.path.join(REF_DIR, "build", "ref_frames")
SUBJECT = os.path.join(REF_DIR, "ref_frames_hip")
STATUS = os.path.join(REF_DIR, "ref_frames.status")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_frames.npz")

# FlakeEncodeParams in flake.h's order: the order of the record's parameter block
PARAM_FIELDS = ("compression", "order_method", "stereo_method", "block_size", "padding_size", "min_prediction_order",
                "max_prediction_order", "prediction_type", "min_partition_order", "max_partition_order",
                "variable_block_size", "allow_vbs")
OM_MAX, OM_EST, OM_2LEVEL, OM_4LEVEL, OM_8LEVEL, OM_SEARCH, OM_LOG = range(7)
PRED_NONE, PRED_FIXED, PRED_LEVINSON = range(3)
FAMILIES = ("levels", "orders", "formats", "stereo", "blocks", "headers", "content", "random")

# flake_set_defaults (encode.c:158-266): what admissible() needs of it -- block size, prediction type, max order,
# variable_block_size, allow_vbs, stereo method
_LEVEL = {lvl: dict(block_size=4096, prediction_type=PRED_LEVINSON, max_prediction_order=8, variable_block_size=0,
                    allow_vbs=0, stereo_method=1) for lvl in range(13)}
for _l in (0, 1, 2):
    _LEVEL[_l].update(block_size=1152, prediction_type=PRED_FIXED, max_prediction_order=(2, 4, 4)[_l])
_LEVEL[0]["stereo_method"] = 0
_LEVEL[3].update(max_prediction_order=6, stereo_method=0)
for _l in range(8, 13):
    _LEVEL[_l]["max_prediction_order"] = 32 if _l >= 11 else 12
    if _l >= 9:
        _LEVEL[_l].update(variable_block_size=1, allow_vbs=1)
    if _l >= 11:
        _LEVEL[_l]["block_size"] = 8192


# ---- signals: integer arithmetic only -----------------------------------------------------------------------

def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _isin(i, period, amp):
    """An integer sine of this period (a multiple of 4) and amplitude: the parabola through its zeros and peaks."""
    h = period // 2
    t = (i % period) - h
    return -(4 * int(amp) * t * (h - np.abs(t))) // (h * h)


def _clip(x, bps):
    a = 1 << (bps - 1)
    return np.clip(x, -a, a - 1).astype(np.int32)


def _small(r, n, bps, div=256):
    a = max((1 << (bps - 1)) // div, 1)
    return r.integers(-a, a + 1, n, dtype=np.int64)


def _base(n, bps, first=0):
    i = np.arange(first, first + n, dtype=np.int64)
    a = 1 << (bps - 1)
    return _isin(i, 200, a // 2) + _isin(i, 52, a // 4) + _isin(i, 1000, a // 8)


def sig_tone(n, ch, bps, seed, block=0):
    """A correlated set: every channel the same three tones, scaled and delayed a little, with noise of its own."""
    r = _rng(seed)
    cols = [(_base(n, bps, 3 * c) * (4 - c % 3)) // 4 + _small(r, n, bps) for c in range(ch)]
    return _clip(np.stack(cols, 1), bps)


def sig_transient(n, ch, bps, seed, block=1024):
    """The tone with every third eighth of a block 36 dB down: something for the variable-block-size split."""
    x = sig_tone(n, ch, bps, seed).astype(np.int64)
    st = max(block // 8, 1)
    quiet = ((np.arange(n) // st) % 3 == 1)
    x[quiet] >>= 6
    return _clip(x, bps)


def sig_noise(n, ch, bps, seed, block=0):
    a = 1 << (bps - 1)
    return _rng(seed).integers(-a, a, (n, ch), dtype=np.int64).astype(np.int32)


def sig_silence(n, ch, bps, seed, block=0):
    return np.zeros((n, ch), np.int32)


def sig_constant_channel(n, ch, bps, seed, block=0):
    x = sig_tone(n, ch, bps, seed)
    x[:, 0] = (1 << (bps - 1)) // 26
    return x


def sig_wasted3(n, ch, bps, seed, block=0):
    return (sig_tone(n, ch, bps, seed) >> 3) << 3


def sig_wasted_one(n, ch, bps, seed, block=0):
    x = sig_tone(n, ch, bps, seed)
    x[:, 0] = (x[:, 0] >> 3) << 3
    return x


def sig_square(n, ch, bps, seed, block=0):
    a = 1 << (bps - 1)
    col = np.where((np.arange(n) // 50) % 2 == 0, a - 1, -a).astype(np.int32)
    return np.stack([col if c % 2 == 0 else -1 - col for c in range(ch)], 1).astype(np.int32)


def sig_quiet_loud(n, ch, bps, seed, block=1024):
    """Blocks quiet, loud (full-scale noise), quiet, ...: the largest frame comes after the first."""
    x = sig_tone(n, ch, bps, seed).astype(np.int64) >> 8
    loud = sig_noise(n, ch, bps, seed + 1)
    odd = ((np.arange(n) // block) % 2 == 1)
    x[odd] = loud[odd]
    return _clip(x, bps)


def sig_l_is_r_plus_noise(n, ch, bps, seed, block=0):
    r = _rng(seed)
    right = _base(n, bps)
    return _clip(np.stack([right + _small(r, n, bps, 64), right], 1), bps)


def sig_r_loud_side_small(n, ch, bps, seed, block=0):
    r = _rng(seed)
    left = _base(n, bps)
    return _clip(np.stack([left, left + _small(r, n, bps, 64)], 1), bps)


def sig_antiphase(n, ch, bps, seed, block=0):
    r = _rng(seed)
    left = _base(n, bps) + _small(r, n, bps, 128)
    return _clip(np.stack([left, -left + _small(r, n, bps, 128)], 1), bps)


def sig_common_plus_own(n, ch, bps, seed, block=0):
    """A common part with noise of its own in either channel: mid and side together are cheapest."""
    r = _rng(seed)
    common = _base(n, bps) // 2 + _small(r, n, bps, 8)
    return _clip(np.stack([common + _small(r, n, bps, 32), common + _small(r, n, bps, 32)], 1), bps)


SIGNALS = {f.__name__[4:]: f for f in (sig_tone, sig_transient, sig_noise, sig_silence, sig_constant_channel,
                                       sig_wasted3, sig_wasted_one, sig_square, sig_quiet_loud,
                                       sig_l_is_r_plus_noise, sig_r_loud_side_small, sig_antiphase,
                                       sig_common_plus_own)}


# ---- the table ----------------------------------------------------------------------------------------------

class Case:
    """One run of the client.  blocks: the call sizes when the caller chooses them, else None (nblocks blocks of
    params.block_size and a tail).  samples_known: FlakeContext.samples is the sample count, else 0."""

    def __init__(self, name, family, level, signal, channels=2, bps=16, rate=44100, nblocks=3, tail=None, blocks=None,
                 samples_known=True, seed=1, shipped=False, **over):
        assert family in FAMILIES and signal in SIGNALS and "compression" not in over
        assert all(k in PARAM_FIELDS for k in over)
        self.name, self.family, self.level, self.signal = name, family, level, signal
        self.channels, self.bps, self.rate = channels, bps, rate
        self.over, self.seed, self.shipped, self.samples_known = dict(over), seed, shipped, samples_known
        self.block_size = over.get("block_size", _LEVEL[level]["block_size"])
        if blocks is None:
            tail = self.block_size // 2 if tail is None else tail
            blocks = [self.block_size] * nblocks + ([tail] if tail else [])
            self.explicit = False
        else:
            self.explicit = True
        self.blocks = [int(b) for b in blocks]

    def setting(self, key):
        return self.over.get(key, _LEVEL[self.level][key])

    @property
    def total(self):
        return sum(self.blocks)

    @property
    def samples(self):
        return self.total if self.samples_known else 0

    @property
    def signal_bits(self):
        """The width the signal is made for: the sample size, but 28 bits in a 32-bit stream (admissible())."""
        return min(self.bps, 28)

    def pcm(self):
        """[total][channels] int32."""
        x = SIGNALS[self.signal](self.total, self.channels, self.signal_bits, self.seed, block=self.block_size)
        assert x.shape == (self.total, self.channels) and x.dtype == np.int32
        return np.ascontiguousarray(x)

    def argv(self, out, pcm_path):
        a = [out, pcm_path, str(self.channels), str(self.rate), str(self.bps), str(self.samples), str(self.level)]
        a += [f"{k}={v}" for k, v in self.over.items()]
        return a + ["blocks=" + ",".join(str(b) for b in self.blocks)]

    def frame_lengths(self):
        """Every length a frame of this case can have: each call's block and, where a block can be split
        (encode.c:997-998), every run of eighths of it."""
        out = set()
        for n in self.blocks:
            out.add(n)
            if self.setting("variable_block_size") and n % 8 == 0 and n >= 128:
                out.update(k * (n // 8) for k in range(1, 8))
        return sorted(out)

    def __repr__(self):
        return f"Case({self.name})"


# the calls the reference refuses (-1), by case; every other call of the table returns a frame
REFUSED_CALLS = {"call_after_tail": [2]}


def admissible(c: Case):
    """None when every frame the case can produce is defined in the reference, else the reason it is not."""
    if c.bps == 32 and c.channels == 2 and c.setting("stereo_method") != 0:
        return "32-bit stereo with stereo estimation: a 33-bit side channel"
    if c.signal_bits > 28:
        return "a signal whose residuals can reach 2^30"
    if c.setting("prediction_type") == PRED_LEVINSON:
        mo = c.setting("max_prediction_order")
        for m in c.frame_lengths():
            if m % 2:
                return f"an LPC frame of odd length {m}"
            if mo > 4 and m <= mo:
                return f"an LPC frame of {m} samples with max order {mo}"
    return None


def strictly_admissible(c: Case):
    """The narrower rule the random family is drawn under: a block is a multiple of 4, the tail is half a block and
    longer than the max order; where blocks can be split, a block is a multiple of 16 and a sixteenth is longer than
    the max order."""
    mo = c.setting("max_prediction_order")
    n = c.block_size
    if c.blocks != [n] * (len(c.blocks) - 1) + [n // 2] or n % 4 or n // 2 <= mo:
        return "blocks and a tail of half a block longer than the max order"
    if c.setting("variable_block_size") and (n % 16 or n // 16 <= mo):
        return "a sixteenth of a block longer than the max order"
    return admissible(c)


def _lpc(min_o, max_o, **kw):
    return dict(prediction_type=PRED_LEVINSON, min_prediction_order=min_o, max_prediction_order=max_o, **kw)


def _table():
    t = []
    # levels at their default block sizes, tails of half a block: under variable block size an eighth of the tail is
    # 256 samples at levels 9 and 10 (max order 12) and 512 at 11 and 12 (max order 32)
    for lvl in range(13):
        for sig in ("tone", "transient", "noise"):
            t.append(Case(f"level{lvl}_{sig}", "levels", lvl, sig, seed=10 + lvl,
                          shipped=(lvl in (5, 10) and sig == "transient") or (lvl == 3 and sig == "noise")))
    # order methods
    names = ("max", "est", "2level", "4level", "8level", "search", "log")
    for om in range(7):
        for lo, hi in ((1, 8), (1, 12), (5, 32), (7, 9), (32, 32)):
            t.append(Case(f"lpc_{names[om]}_{lo}_{hi}", "orders", 5, "tone", tail=256, seed=40 + om,
                          block_size=1024, order_method=om, **_lpc(lo, hi)))
    for om in (OM_MAX, OM_EST, OM_SEARCH):
        for lo, hi in ((0, 4), (2, 2), (3, 4)):
            t.append(Case(f"fixed_{names[om]}_{lo}_{hi}", "orders", 5, "tone", tail=255, seed=50 + om, block_size=1024,
                          order_method=om, prediction_type=PRED_FIXED, min_prediction_order=lo,
                          max_prediction_order=hi))
    t.append(Case("prediction_none", "orders", 5, "tone", tail=255, block_size=1024, prediction_type=PRED_NONE))
    for lo, hi in ((0, 0), (0, 8), (8, 8), (3, 5)):
        t.append(Case(f"partitions_{lo}_{hi}", "orders", 5, "transient", tail=256, seed=60, block_size=1024,
                      min_partition_order=lo, max_partition_order=hi))
    # formats, at a fixed-block level and at a variable-block one
    for ch, bps in ((1, 8), (1, 16), (2, 12), (2, 20), (2, 24), (3, 24), (6, 20), (8, 16), (1, 32), (3, 32), (2, 32)):
        st = dict(stereo_method=0) if (ch, bps) == (2, 32) else {}
        t.append(Case(f"format_{ch}ch_{bps}bit_level5", "formats", 5, "tone", ch, bps, tail=512, seed=70 + ch,
                      block_size=1024, shipped=(ch, bps) in ((8, 16),), **st))
        t.append(Case(f"format_{ch}ch_{bps}bit_level9", "formats", 9, "transient", ch, bps, tail=512, seed=80 + ch,
                      block_size=1024, **st))
    t.append(Case("format_1ch_24bit_level8", "formats", 8, "tone", 1, 24, tail=512, seed=90, block_size=2048, shipped=True))
    # stereo decisions
    for sig in ("l_is_r_plus_noise", "r_loud_side_small", "antiphase", "common_plus_own", "noise"):
        for sm in (0, 1):
            t.append(Case(f"stereo_{sig}_method{sm}", "stereo", 5, sig, tail=512, seed=100, block_size=1024,
                          stereo_method=sm))
    # block sizes; LPC where the reference defines it, the fixed predictor for the odd size
    for n in (16, 32, 192, 256, 1000, 1152, 4096, 4608, 5000):
        t.append(Case(f"block_{n}_lpc", "blocks", 5, "tone", tail=12 if n == 16 else n // 2 + (n // 2) % 2, seed=110,
                      block_size=n))
        t.append(Case(f"block_{n}_fixed", "blocks", 2, "transient", tail=n // 2 - 1, seed=111, block_size=n))
    t.append(Case("block_16384_lpc", "blocks", 8, "tone", nblocks=1, tail=0, seed=112, block_size=16384))
    t.append(Case("block_16384_vbs", "blocks", 9, "transient", nblocks=1, tail=0, seed=113, block_size=16384))
    t.append(Case("block_65535_fixed", "blocks", 2, "tone", nblocks=1, tail=0, seed=114, block_size=65535))
    own = [4096, 1024, 2048, 256, 160, 1004, 4096, 192]
    t.append(Case("caller_blocks_whole", "blocks", 5, "transient", blocks=own, seed=115, allow_vbs=1))
    t.append(Case("caller_blocks_split", "blocks", 5, "transient", blocks=own, seed=115, allow_vbs=1,
                  variable_block_size=1))
    for tail in (1, 15, 1151):
        t.append(Case(f"tail_{tail}", "blocks", 1, "tone", tail=tail, seed=116))
    # headers
    for rate in (44100, 96000, 192000, 64000, 12345, 44110):
        t.append(Case(f"rate_{rate}", "headers", 5, "tone", rate=rate, tail=512, seed=120, block_size=1024,
                      shipped=rate == 12345))
    t.append(Case("frames_130_mono", "headers", 5, "tone", 1, nblocks=130, tail=0, seed=121, block_size=16,
                  shipped=True))
    t.append(Case("vbs_past_65536", "headers", 9, "transient", 1, nblocks=17, tail=1024, seed=122))
    t.append(Case("samples_unknown", "headers", 5, "tone", tail=512, seed=123, block_size=1024, samples_known=False,
                  shipped=True))
    # a call behind the short block of a fixed-block stream is refused (the last_frame latch, encode.c:991-994)
    t.append(Case("call_after_tail", "headers", 5, "tone", blocks=[1024, 512, 1024], seed=125, block_size=1024))
    t.append(Case("padding_0", "headers", 5, "tone", tail=512, seed=124, block_size=1024, padding_size=0))
    # content
    for sig in ("silence", "constant_channel", "wasted3", "wasted_one", "square", "quiet_loud"):
        t.append(Case(f"content_{sig}", "content", 5, sig, tail=512, seed=130, block_size=1024))
        t.append(Case(f"content_{sig}_level10", "content", 10, sig, tail=512, seed=131, block_size=1024))
    t.append(Case("content_quiet_loud_24bit_mono", "content", 6, "quiet_loud", 1, 24, nblocks=4, tail=512, seed=132,
                  block_size=1024))
    t += _random_cases(RANDOM_COUNT)
    return t


RANDOM_COUNT = 512


def _random_cases(count):
    """Seeded parameter sets over the ranges above, drawn until `count` are strictly admissible and valid."""
    r = _rng(20240)
    out = []
    sigs = ("tone", "transient", "noise", "wasted3", "wasted_one", "quiet_loud", "square", "common_plus_own",
            "constant_channel", "antiphase")
    while len(out) < count:
        lvl = int(r.integers(0, 13))
        ch = int((1, 2, 2, 2, 3, 4, 6, 8)[r.integers(0, 8)])
        bps = int((8, 12, 16, 16, 20, 24, 32)[r.integers(0, 7)])
        over = {}
        pred = int(r.integers(0, 3)) if r.integers(0, 2) else _LEVEL[lvl]["prediction_type"]
        over["prediction_type"] = pred
        top = 4 if pred == PRED_FIXED else 32
        low = 0 if pred == PRED_FIXED else 1
        hi = int(r.integers(low, top + 1)) if pred != PRED_LEVINSON or r.integers(0, 2) else int(r.integers(1, 13))
        over["max_prediction_order"] = hi
        over["min_prediction_order"] = int(r.integers(low, hi + 1))
        over["order_method"] = int(r.integers(0, 7))
        over["stereo_method"] = int(r.integers(0, 2))
        pmax = int(r.integers(0, 9))
        over["max_partition_order"] = pmax
        over["min_partition_order"] = int(r.integers(0, pmax + 1))
        allow = int(r.integers(0, 2))
        over["allow_vbs"] = allow
        over["variable_block_size"] = int(r.integers(0, 2)) if allow else 0
        over["block_size"] = int(16 * r.integers(8 if allow else 1, 129))
        over["padding_size"] = int(r.integers(0, 65))
        sig = sigs[int(r.integers(0, len(sigs)))]
        if ch != 2 and sig in ("common_plus_own", "antiphase"):
            sig = "tone"
        c = Case(f"random{len(out):03d}", "random", lvl, sig, ch, bps, rate=int((44100, 48000, 8000, 22222)[r.integers(0, 4)]),
                 nblocks=2, seed=1000 + len(out), samples_known=bool(r.integers(0, 2)), **over)
        if strictly_admissible(c) is None:
            out.append(c)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _table()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def case(name) -> Case:
    return next(c for c in cases() if c.name == name)


def gpu_cases():
    """The in-process GPU leg's cases: all but the random family."""
    return [c for c in cases() if c.family != "random"]


def pcm_sha1(pcm) -> bytes:
    return hashlib.sha1(np.ascontiguousarray(pcm, "<i4").tobytes()).digest()


# ---- record files -------------------------------------------------------------------------------------------

class Record:
    """What one run of the client wrote (oracle/ref_frames.c states the layout)."""

    def __init__(self, data: bytes):
        assert data[:4] == b"FRF1", "not a ref_frames record"
        self.raw = data
        at = [4]

        def i32():
            at[0] += 4
            return struct.unpack_from("<i", data, at[0] - 4)[0]

        def take(n):
            at[0] += n
            assert at[0] <= len(data), "truncated record"
            return data[at[0] - n:at[0]]

        self.valid = i32()
        self.params = {k: i32() for k in PARAM_FIELDS}
        self.header_len, self.header, self.calls, self.si_rc, self.streaminfo = -1, b"", [], -1, b""
        if self.valid < 0:
            return
        self.header_len = i32()
        self.header = take(max(self.header_len, 0))
        for _ in range(i32()):
            n, rc = i32(), i32()
            self.calls.append((n, rc, take(max(rc, 0))))
        self.si_rc = i32()
        self.streaminfo = take(34)
        assert at[0] == len(data), "bytes behind the record's end"


def run_client(program, c: Case, pcm=None, env=None, timeout=60) -> Record:
    """One fresh child process of the witness or the subject on this case; a non-zero exit is an error."""
    pcm = c.pcm() if pcm is None else pcm
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "pcm.raw"), os.path.join(d, "record.bin")
        np.ascontiguousarray(pcm, "<i4").tofile(src)
        r = subprocess.run([program] + c.argv(out, src), capture_output=True, timeout=timeout, env=env)
        if r.returncode != 0:
            raise RuntimeError(f"{os.path.basename(program)} on {c.name}: exit {r.returncode}: "
                               f"{r.stderr.decode(errors='replace')[-2000:]}")
        with open(out, "rb") as f:
            return Record(f.read())


def witness_state():
    """'live' where the witness is built, 'recorded' where no reference build was attempted; raises where one was
    attempted and left no witness (oracle/Makefile writes its verdict into oracle/_ref/ref_frames.status)."""
    if os.path.exists(STATUS):
        with open(STATUS) as f:
            verdict = f.read().strip()
        if verdict != "built" or not os.path.exists(WITNESS):
            raise AssertionError(f"oracle/Makefile refframes: {verdict!r} -- the reference tree was there and the witness "
                                 "was not built; see the build's output")
        return "live"
    return "live" if os.path.exists(WITNESS) else "recorded"


# ---- frames: boundaries by the project's indexer, contents by the format ------------------------------------

CH_NAMES = {8: "left/side", 9: "right/side", 10: "mid/side"}


def split_frames(call_bytes: bytes, streaminfo34: bytes):
    """The frames one flake_encode_frame() call returned, cut apart by the project's own frame-header parser and
    indexer (flake_amd.index_frames: flac_header.h's predicate and the CRC-16)."""
    import flake_amd
    si, _ = flake_amd.read_streaminfo(streaminfo34)
    got = flake_amd.index_frames(si, call_bytes)
    assert got is not None, "the call's bytes do not begin with a frame of this stream"
    sizes, used = got
    assert used == len(call_bytes), f"frames cover {used} of the call's {len(call_bytes)} bytes"
    out, off = [], 0
    for s in sizes:
        out.append(call_bytes[off:off + int(s)])
        off += int(s)
    return out


def header_fields(frame: bytes) -> dict:
    """A frame header's raw codes, for coverage conditions and for reports."""
    b0 = frame[4]
    ones = 0
    while (b0 << ones) & 0x80:
        ones += 1
    nbytes = max(ones, 1)
    number = b0 & (0xFF >> (ones + 1)) if ones else b0
    for b in frame[5:4 + nbytes]:
        number = number << 6 | (b & 63)
    bs_code = frame[2] >> 4
    p = 4 + nbytes
    n = None
    if bs_code == 6:
        n = frame[p] + 1
    elif bs_code == 7:
        n = (frame[p] << 8 | frame[p + 1]) + 1
    return dict(vbs=frame[1] & 1, bs_code=bs_code, sr_code=frame[2] & 15, ch_code=frame[3] >> 4,
                bps_code=(frame[3] >> 1) & 7, number=number, number_bytes=nbytes, explicit_n=n, size=len(frame))


# one feature word per frame, kept in the record: what the coverage conditions of the GPU leg are computed from
F_CONSTANT, F_VERBATIM, F_FIXED, F_LPC, F_WASTED = 1, 2, 4, 8, 16
FEATURE_DTYPE = np.dtype([("bs_code", "u1"), ("sr_code", "u1"), ("ch_code", "u1"), ("number_bytes", "u1"),
                          ("subframes", "u1"), ("vbs", "u1"), ("n", "<u2")])


def frame_features(frame: bytes, channels: int, bps: int):
    from test_format_edges_cpu import parse_frame
    h, subs = parse_frame(frame, channels, bps)
    f = np.zeros((), FEATURE_DTYPE)
    hf = header_fields(frame)
    for k in ("bs_code", "sr_code", "ch_code", "number_bytes", "vbs"):
        f[k] = hf[k]
    f["n"] = h["n"]
    bits = {"constant": F_CONSTANT, "verbatim": F_VERBATIM, "fixed": F_FIXED, "lpc": F_LPC}
    f["subframes"] = int(np.bitwise_or.reduce([bits[s["type"]] | (F_WASTED if s["wasted"] else 0) for s in subs]))
    return f


def describe(frame: bytes) -> str:
    h = header_fields(frame)
    ch = CH_NAMES.get(h["ch_code"], f"{h['ch_code'] + 1} independent")
    return (f"{h['size']} bytes, block-size code {h['bs_code']}" + (f" (n = {h['explicit_n']})" if h["explicit_n"] else "")
            + f", rate code {h['sr_code']}, channels {ch}, size code {h['bps_code']}, "
            + ("sample" if h["vbs"] else "frame") + f" number {h['number']}")


def first_difference(got_calls, exp_calls, streaminfo34, what=("got", "expected")):
    """None when the calls' return values and bytes are equal, else a report that names the first differing call and
    frame with both headers' fields."""
    if len(got_calls) != len(exp_calls):
        return f"{len(got_calls)} calls against {len(exp_calls)}"
    for i, ((gn, grc, gb), (en, erc, eb)) in enumerate(zip(got_calls, exp_calls)):
        if (gn, grc, gb) == (en, erc, eb):
            continue
        msg = f"call {i} (block of {en}): {what[0]} returned {grc}, {what[1]} {erc}"
        try:
            gf, ef = split_frames(gb, streaminfo34), split_frames(eb, streaminfo34)
        except AssertionError as e:
            return msg + f"; frames not separable ({e})"
        if len(gf) != len(ef):
            msg += f"; {len(gf)} frames against {len(ef)}"
        for k, (a, b) in enumerate(zip(gf, ef)):
            if a != b:
                at = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
                return msg + f"; frame {k} of the call differs at byte {at}: {what[0]} [{describe(a)}], {what[1]} [{describe(b)}]"
        return msg
    return None


# ---- the golden record --------------------------------------------------------------------------------------

def golden_entry(c: Case, rec: Record, pcm):
    """What the record keeps of one run: no frame bodies.  The random family, which only the CPU leg runs, keeps no
    feature words."""
    frames_per_call, sha, feat = [], [], []
    for n, rc, data in rec.calls:
        fr = split_frames(data, rec.streaminfo) if rc > 0 else []
        frames_per_call.append(len(fr))
        for f in fr:
            sha.append(np.frombuffer(hashlib.sha1(f).digest(), np.uint8))
            if c.family != "random":
                feat.append(frame_features(f, c.channels, c.bps))
    return dict(valid=rec.valid, params=np.array([rec.params[k] for k in PARAM_FIELDS], np.int32),
                pcmsha=np.frombuffer(pcm_sha1(pcm), np.uint8), header=np.frombuffer(rec.header, np.uint8),
                call_n=np.array([n for n, _, _ in rec.calls], np.int32),
                call_ret=np.array([rc for _, rc, _ in rec.calls], np.int32),
                call_frames=np.array(frames_per_call, np.int32),
                frame_sha=np.stack(sha) if sha else np.zeros((0, 20), np.uint8),
                frame_feat=np.array(feat, FEATURE_DTYPE) if feat else np.zeros(0, FEATURE_DTYPE),
                si_rc=rec.si_rc, streaminfo=np.frombuffer(rec.streaminfo, np.uint8))


_KEYS = ("params", "pcmsha", "header", "call_n", "call_ret", "call_frames", "frame_sha", "frame_feat", "streaminfo")


def save_golden(entries: dict, path=GOLDEN):
    """entries: name -> golden_entry.  Stored as a few long arrays with per-case lengths."""
    names = sorted(entries)
    save = {"source": "oracle/_ref/build/ref_frames: the reference's own libflake (its CMake build) under oracle/ref_frames.c",
            "names": np.array(names), "valid": np.array([entries[n]["valid"] for n in names], np.int32),
            "si_rc": np.array([entries[n]["si_rc"] for n in names], np.int32)}
    for k in _KEYS:
        parts = [entries[n][k] for n in names]
        save[k] = np.concatenate(parts)
        save[k + "_len"] = np.array([len(p) for p in parts], np.int32)
    np.savez_compressed(path, **save)


_GOLDEN = None


def load_golden(path=GOLDEN) -> dict:
    global _GOLDEN
    if _GOLDEN is None or path != GOLDEN:
        z = np.load(path, allow_pickle=False)
        names = [str(n) for n in z["names"]]
        out = {n: dict(valid=int(z["valid"][i]), si_rc=int(z["si_rc"][i])) for i, n in enumerate(names)}
        for k in _KEYS:
            offs = np.concatenate([[0], np.cumsum(z[k + "_len"], dtype=np.int64)])
            arr = z[k]
            for i, n in enumerate(names):
                out[n][k] = arr[offs[i]:offs[i + 1]]
        if path != GOLDEN:
            return out
        _GOLDEN = out
    return _GOLDEN


def entry_difference(got: dict, exp: dict):
    """None when two golden entries say the same, else the first field that differs."""
    for k in ("valid", "si_rc"):
        if int(got[k]) != int(exp[k]):
            return f"{k}: {got[k]} against {exp[k]}"
    for k in _KEYS:
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            if k == "params":
                bad = [f"{f} {int(x)} against {int(y)}" for f, x, y in zip(PARAM_FIELDS, a, b) if x != y]
                return "effective parameters: " + ", ".join(bad)
            if k == "frame_sha" and a.shape == b.shape:
                return f"frame {int(np.nonzero((a != b).any(1))[0][0])} of the stream has other bytes"
            return f"{k} differs ({a.shape} against {b.shape})"
    return None


# ---- metadata: the bytes before the first frame --------------------------------------------------------------

# What a stream of this project may say differently from the reference's, by name.  Anything else must be equal.
METADATA_ALLOWED = {"vendor string": "the VORBIS_COMMENT block names the library that wrote the stream "
                                     "(metadata.c:94 \"Flake SVN\"; flake_host.c \"flake-amd 0.1\")"}
METADATA_ALLOWED["provisional MD5"] = (
    "the MD5 field of the STREAMINFO that flake_encode_init() writes before any block: the reference finalises an MD5 "
    "context it has not yet initialised (encode.c:461 before :469), this project the MD5 of no samples; every client "
    "rewrites the block at the end, and the final STREAMINFO must be equal")
BLOCK_NAMES = {0: "STREAMINFO", 1: "PADDING", 3: "SEEKTABLE", 4: "VORBIS_COMMENT"}


def metadata_blocks(data: bytes):
    """([(last, type, body)], offset of the first byte behind the last block) of a stream that starts with "fLaC"."""
    assert data[:4] == b"fLaC", "no stream marker"
    pos, out, last = 4, [], 0
    while not last:
        assert pos + 4 <= len(data), "metadata runs past the end"
        last, typ = data[pos] >> 7, data[pos] & 0x7F
        ln = int.from_bytes(data[pos + 1:pos + 4], "big")
        out.append((last, typ, bytes(data[pos + 4:pos + 4 + ln])))
        pos += 4 + ln
    return out, pos


def _comment_parts(body: bytes):
    vlen = int.from_bytes(body[:4], "little")
    return body[4:4 + vlen], body[4 + vlen:]


def metadata_differences(got: bytes, exp: bytes, streaminfo=True):
    """The named differences between two streams' metadata: a subset of METADATA_ALLOWED's names when all is well.
    streaminfo False is for the header flake_encode_init() returns: its STREAMINFO's MD5 field is named on its own."""
    gb, gend = metadata_blocks(got)
    eb, eend = metadata_blocks(exp)
    diffs = []
    if [(l, t) for l, t, _ in gb] != [(l, t) for l, t, _ in eb]:
        return [f"block sequence {[(l, BLOCK_NAMES.get(t, t)) for l, t, _ in gb]} against "
                f"{[(l, BLOCK_NAMES.get(t, t)) for l, t, _ in eb]}"]
    for (_, typ, g), (_, _, e) in zip(gb, eb):
        name = BLOCK_NAMES.get(typ, str(typ))
        if typ == 0 and not streaminfo:
            if g[:18] != e[:18]:
                diffs.append("STREAMINFO content before the MD5")
            elif g[18:] != e[18:]:
                diffs.append("provisional MD5")
            continue
        if typ == 4:
            (gv, grest), (ev, erest) = _comment_parts(g), _comment_parts(e)
            if gv != ev:
                diffs.append("vendor string")
            if grest != erest:
                diffs.append("VORBIS_COMMENT entries")
        elif len(g) != len(e):
            diffs.append(f"{name} length {len(g)} against {len(e)}")
        elif g != e:
            diffs.append(f"{name} content")
    return diffs
