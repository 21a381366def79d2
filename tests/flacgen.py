"""A small pure-Python FLAC frame writer for the verifier's tests.

It writes frames in forms this project's encoder never emits -- every subframe type, FIXED 0-4 and
LPC 1-32, wasted bits, RICE and RICE2, escape partitions (raw width 0 included), every channel
assignment, explicit block-size and sample-rate codes, long UTF-8 numbers -- straight from the FLAC
format.  Samples are restored the way libFLAC does (64-bit prediction sum, arithmetic shift, int32
wrap), so the residual written here is the one a decoder needs.

catalogue() and utf8_catalogue() hold every form once; edge_catalogue() holds frames built around the limits at
which the verifier and the decoder change path (partition groups, residency, staging, block sizes, widths).
"""
from __future__ import annotations

import numpy as np

FIXED_COEFS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12,
            8192: 13, 16384: 14, 32768: 15}
SR_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9,
            48000: 10, 96000: 11}
BPS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


class BitWriter:
    def __init__(self):
        self.bits: list[int] = []

    def put(self, nb: int, v: int) -> None:
        if nb:
            self.bits.extend(map(int, format(v & ((1 << nb) - 1), "b").zfill(nb)))

    def unary(self, q: int) -> None:
        self.bits.extend([0] * q)
        self.bits.append(1)

    def align(self) -> None:
        while len(self.bits) % 8:
            self.bits.append(0)

    def nbits(self) -> int:
        return len(self.bits)

    def tobytes(self) -> bytes:
        assert len(self.bits) % 8 == 0
        a = np.array(self.bits, dtype=np.uint8).reshape(-1, 8)
        return bytes(np.packbits(a, axis=1).ravel())


def utf8(v: int) -> bytes:
    """The UTF-8 style coded number, 1 to 7 bytes (up to 36 bits)."""
    if v < 0x80:
        return bytes([v])
    for nbytes in range(2, 8):
        payload = 6 * (nbytes - 1) + (7 - nbytes if nbytes < 7 else 0)
        if v < (1 << payload):
            out = []
            for _ in range(nbytes - 1):
                out.append(0x80 | (v & 0x3F))
                v >>= 6
            first = ((0xFF00 >> nbytes) & 0xFF) | v
            return bytes([first] + out[::-1])
    raise ValueError("number needs more than 36 bits")


def zigzag(e: int) -> int:
    return (e << 1) if e >= 0 else ((-e) << 1) - 1


def channel_values(pcm: np.ndarray, ch_code: int) -> list[np.ndarray]:
    """The subframes' values (int64) for a frame's channel assignment."""
    x = pcm.astype(np.int64)
    if ch_code < 8:
        return [x[:, c] for c in range(x.shape[1])]
    l, r = x[:, 0], x[:, 1]
    if ch_code == 8:
        return [l, l - r]
    if ch_code == 9:
        return [l - r, r]
    return [(l + r) >> 1, l - r]


def prediction(y: np.ndarray, kind: str, order: int, coefs=None, shift: int = 0):
    """(acc, pred) as int64 arrays for samples i >= order: the 64-bit sum over the history and what a decoder adds to
    the residual (FIXED: the sum itself; LPC: the sum shifted down, arithmetically).  No sum here leaves int64: 32
    taps of 15 bits on 33-bit values stay below 2^53."""
    y = np.asarray(y, np.int64)
    cs = FIXED_COEFS[order] if kind == "fixed" else [int(c) for c in coefs]
    acc = np.zeros(len(y) - order, np.int64)
    for j, c in enumerate(cs):
        acc += c * y[order - 1 - j:len(y) - 1 - j]
    return acc, (acc if kind == "fixed" else acc >> shift)


def residual(y: np.ndarray, kind: str, order: int, coefs=None, shift: int = 0) -> list[int]:
    """e[i] for i >= order, int32-wrapped as a decoder restores them."""
    y = np.asarray(y, np.int64)
    _, pred = prediction(y, kind, order, coefs, shift)
    e = (y[order:] - pred) & 0xFFFFFFFF
    return [int(v) for v in np.where(e >= 1 << 31, e - (1 << 32), e)]


def minbits_signed(vals) -> int:
    m = 0
    for v in vals:
        b = (v.bit_length() + 1) if v >= 0 else ((-v - 1).bit_length() + 1)
        m = max(m, b if v != 0 else 0)
    return m


def put_residual(w: BitWriter, res: list[int], n: int, order: int, method: int, porder: int,
                 escape=(), ks=None, offsets=None) -> None:
    """escape: partitions written raw ("escape partitions"); ks: Rice parameter per partition (None: a
    simple estimate); offsets: a list that takes the bit offset at which each residual's codeword starts (and, last,
    the offset behind the last one)."""
    w.put(2, method)
    w.put(4, porder)
    pbits, esc = (5, 31) if method else (4, 15)
    psz = n >> porder
    i = 0
    for j in range(1 << porder):
        cnt = psz - (order if j == 0 else 0)
        part = res[i:i + cnt]
        i += cnt
        if j in escape:
            raw = minbits_signed(part)
            assert raw < 32, "a raw field holds at most 31 bits"
            w.put(pbits, esc)
            w.put(5, raw)
            for e in part:
                if offsets is not None:
                    offsets.append(w.nbits())
                w.put(raw, e)
            continue
        if ks is not None:
            k = ks[j]
        else:
            mean = sum(zigzag(e) for e in part) / max(1, len(part))
            k = max(0, int(mean).bit_length() - 1)
        k = min(k, esc - 1)
        w.put(pbits, k)
        if len(part) >= 32:
            # the same bits as the loop below, all codewords of the partition at once: q zeros, a one, k bits
            e = np.array(part, np.int64)
            u = np.where(e >= 0, e << 1, ((-e) << 1) - 1)
            q = u >> k
            ln = q + 1 + k
            one = np.cumsum(ln) - ln + q
            bits = np.zeros(int(ln.sum()), np.uint8)
            bits[one] = 1
            for b in range(k):
                bits[one + 1 + b] = (u >> (k - 1 - b)) & 1
            if offsets is not None:
                offsets.extend((w.nbits() + one - q).tolist())
            w.bits.extend(bits.tolist())
            continue
        for e in part:
            if offsets is not None:
                offsets.append(w.nbits())
            u = zigzag(e)
            w.unary(u >> k)
            w.put(k, u & ((1 << k) - 1))
    if offsets is not None:
        offsets.append(w.nbits())


def put_subframe(w: BitWriter, y: np.ndarray, bps: int, spec: dict, offsets=None) -> None:
    """spec: kind (constant | verbatim | fixed | lpc), order, coefs, precision, shift, wasted, method,
    porder, escape, ks.  offsets: put_residual's (FIXED and LPC only)."""
    kind = spec["kind"]
    wasted = spec.get("wasted", 0)
    if wasted:
        assert not np.any(y & ((1 << wasted) - 1)), "samples have fewer wasted bits"
        y = y >> wasted
    wb = bps - wasted
    n = len(y)
    order = spec.get("order", 0)
    code = {"constant": 0, "verbatim": 1}.get(kind)
    if code is None:
        code = 8 + order if kind == "fixed" else 31 + order
    w.put(1, 0)
    w.put(6, code)
    if wasted:
        w.put(1, 1)
        w.unary(wasted - 1)
    else:
        w.put(1, 0)
    if kind == "constant":
        assert np.all(y == y[0])
        w.put(wb, int(y[0]))
        return
    if kind == "verbatim":
        for v in y:
            w.put(wb, int(v))
        return
    for v in y[:order]:
        w.put(wb, int(v))
    coefs, shift = None, 0
    if kind == "lpc":
        prec = spec["precision"]
        coefs, shift = spec["coefs"], spec["shift"]
        w.put(4, prec - 1)
        w.put(5, shift)
        for c in coefs:
            w.put(prec, c)
    res = residual(y, kind, order, coefs, shift)
    put_residual(w, res, n, order, spec.get("method", 0), spec.get("porder", 0), spec.get("escape", ()),
                 spec.get("ks"), offsets)


def frame(pcm: np.ndarray, number: int, bps: int, sample_rate: int, subframes: list[dict], ch_code=None,
          vbs: bool = False, bs_code=None, sr_code=None, bps_code=None, offsets=None) -> bytes:
    """One frame of pcm ([n][channels] int32).  number: the frame number (fixed blocks) or the first sample
    (vbs).  bs_code / sr_code / bps_code: force a header code (6 / 7, 12 / 13 / 14 carry the value).  offsets: a list
    that takes, per subframe, put_residual's list of codeword offsets (bits from the frame's start)."""
    n, nch = pcm.shape
    if ch_code is None:
        ch_code = nch - 1
    if bs_code is None:
        bs_code = BS_CODES.get(n, 6 if n <= 256 else 7)
    if sr_code is None:
        sr_code = SR_CODES.get(sample_rate, 0)
    if bps_code is None:
        bps_code = BPS_CODES.get(bps, 0)
    w = BitWriter()
    w.put(14, 0x3FFE)
    w.put(1, 0)
    w.put(1, 1 if vbs else 0)
    w.put(4, bs_code)
    w.put(4, sr_code)
    w.put(4, ch_code)
    w.put(3, bps_code)
    w.put(1, 0)
    for b in utf8(number):
        w.put(8, b)
    if bs_code == 6:
        w.put(8, n - 1)
    elif bs_code == 7:
        w.put(16, n - 1)
    if sr_code == 12:
        w.put(8, sample_rate // 1000)
    elif sr_code == 13:
        w.put(16, sample_rate)
    elif sr_code == 14:
        w.put(16, sample_rate // 10)
    w.put(8, crc8(w.tobytes()))
    vals = channel_values(pcm, ch_code)
    for c, spec in enumerate(subframes):
        side = (ch_code == 8 and c == 1) or (ch_code == 9 and c == 0) or (ch_code == 10 and c == 1)
        offs = None
        if offsets is not None:
            offs = []
            offsets.append(offs)
        put_subframe(w, vals[c], bps + (1 if side else 0), spec, offs)
    w.align()
    body = w.tobytes()
    return body + crc16(body).to_bytes(2, "big")


def lpc_coefs(order: int, precision: int = 12, seed: int = 0):
    """A stable-ish predictor (quantised taps of a decaying sinc) with its shift."""
    rng = np.random.default_rng(seed)
    taps = np.array([(0.9 ** j) * (1.0 if j == 0 else 0.3 * rng.standard_normal()) for j in range(order)])
    shift = precision - 2
    q = np.clip(np.round(taps * (1 << shift)), -(1 << (precision - 1)), (1 << (precision - 1)) - 1).astype(int)
    return [int(v) for v in q], shift


def test_signal(n: int, nch: int, bps: int, seed: int = 0, wasted: int = 0) -> np.ndarray:
    """A smooth signal with noise, [n][nch] int32 within bps bits (the low `wasted` bits zero)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    amp = (1 << (bps - 2)) - 1
    out = np.zeros((n, nch), np.int64)
    for c in range(nch):
        s = amp * 0.6 * np.sin(2 * np.pi * t * (0.003 + 0.002 * c)) + rng.normal(0, amp * 0.01 + 1, n)
        out[:, c] = np.clip(np.round(s), -amp, amp).astype(np.int64)
    if wasted:
        out = (out >> wasted) << wasted
    return out.astype(np.int32)


def catalogue(bps: int = 16, sample_rate: int = 44100):
    """(name, pcm, frame bytes, bps, sample_rate, channels) for every form the verifier must accept; frame
    numbers count from 0 in each (a stream of one frame each)."""
    out = []

    def add(name, pcm, subs, bps_=bps, sr=sample_rate, **kw):
        out.append((name, pcm, frame(pcm, kw.pop("number", 0), bps_, sr, subs, **kw), bps_, sr, pcm.shape[1]))

    n = 1152
    x = test_signal(n, 2, bps, seed=1)
    mono = x[:, :1].copy()
    add("constant", np.full((n, 1), -77, np.int32), [dict(kind="constant")])
    add("constant_zero", np.zeros((n, 1), np.int32), [dict(kind="constant")])
    add("verbatim", mono, [dict(kind="verbatim")])
    for o in range(5):
        add(f"fixed{o}", mono, [dict(kind="fixed", order=o, porder=2)])
    for o in (1, 2, 8, 12, 31, 32):
        coefs, shift = lpc_coefs(o, 12, seed=o)
        add(f"lpc{o}", mono, [dict(kind="lpc", order=o, coefs=coefs, precision=12, shift=shift, porder=3)])
    coefs, shift = lpc_coefs(4, 15, seed=9)
    add("lpc4_prec15", mono, [dict(kind="lpc", order=4, coefs=coefs, precision=15, shift=shift, porder=0)])
    add("lpc2_shift0", mono, [dict(kind="lpc", order=2, coefs=[1, 0], precision=2, shift=0, porder=1)])
    add("rice2", mono, [dict(kind="fixed", order=2, method=1, porder=4)])
    add("rice2_bigk", mono, [dict(kind="fixed", order=1, method=1, porder=0, ks=[20])])
    add("escape", mono, [dict(kind="fixed", order=2, porder=3, escape=(0, 3, 7))])
    add("escape_rice2", mono, [dict(kind="fixed", order=2, method=1, porder=2, escape=(1,))])
    z = mono.copy()
    z[:300] = 5
    add("escape_raw0", z, [dict(kind="fixed", order=1, porder=2, escape=(0,))])
    add("wasted", test_signal(n, 1, bps, seed=3, wasted=3), [dict(kind="fixed", order=2, wasted=3, porder=2)])
    add("wasted_verbatim", test_signal(n, 1, bps, seed=4, wasted=1), [dict(kind="verbatim", wasted=1)])
    st = [dict(kind="fixed", order=2, porder=2), dict(kind="fixed", order=1, porder=2)]
    add("ch_independent", x, st, ch_code=1)
    for cc in (8, 9, 10):
        add(f"ch{cc}", x, st, ch_code=cc)
    add("ch10_lpc", x, [dict(kind="lpc", order=8, coefs=lpc_coefs(8)[0], precision=12, shift=lpc_coefs(8)[1],
                             porder=4), dict(kind="verbatim")], ch_code=10)
    m = 1000
    y = test_signal(m, 1, bps, seed=5)
    add("bs_explicit16", y, [dict(kind="fixed", order=2, porder=3)], bs_code=7)
    add("bs_explicit8", y[:200], [dict(kind="fixed", order=2, porder=3)], bs_code=6)
    add("bs_table_as_explicit", mono[:192], [dict(kind="fixed", order=1, porder=0)], bs_code=7)
    add("sr_khz", mono, [dict(kind="fixed", order=1)], sr=48000, sr_code=12)
    add("sr_hz", mono, [dict(kind="fixed", order=1)], sr=44100, sr_code=13)
    add("sr_tens", mono, [dict(kind="fixed", order=1)], sr=44100, sr_code=14)
    add("sr_streaminfo", mono, [dict(kind="fixed", order=1)], sr_code=0)
    add("bps_streaminfo", mono, [dict(kind="fixed", order=1)], bps_code=0)
    return out


def utf8_catalogue(bps: int = 16):
    """Frames whose numbers take 5, 6 and 7 bytes (sample numbers of a variable-block-size stream)."""
    n = 256
    pcm = test_signal(n, 1, bps, seed=11)
    out = []
    for first in ((1 << 21) + 3, (1 << 26) + 5, (1 << 31) + 7, (1 << 35) + 9):
        out.append((first, pcm, frame(pcm, first, bps, 44100, [dict(kind="fixed", order=2, porder=1)], vbs=True)))
    return out


# ---- frames at the kernels' internal limits ----------------------------------------------------------------

# The limits of K5 (k5_verify.hip) and K7 (k7_decode.hip) the cases below are built around; the tests assert each case's
# property against these from the frame's bytes.
K5_MAX_PARTS = 256        # partitions per group of K5's walk
K5_RES_CAP = 4608         # blocks up to this are resident in K5's LDS
K5_FB_CAP = 12288         # frames up to this many bytes are staged in K5's LDS
K7_DFB_CAP = 16384        # ... in K7's
K7_CHUNK = 64             # K7 hands over this many restored samples at a time
K7_RING = 128             # ... out of a ring of this many


class Edge:
    """One case of edge_catalogue(): group ('a' .. 'f'), name, pcm [n][channels] int32, frame (the bytes of all its
    frames), frame_bytes (their sizes), blocks (their samples), bps, rate, channels, vbs (variable block size: frames numbered by first
    sample), prop (what the case was built for, see edge_catalogue), subs / ch_code (how the first frame was written)
    and offsets (per subframe of the first frame, put_residual's codeword offsets)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return len(self.pcm)

    def __repr__(self):
        return f"Edge({self.group}:{self.name})"


def quiet_signal(n: int, nch: int, seed: int, amp: int = 200, noise: int = 2) -> np.ndarray:
    """A slow sine of small amplitude with uniform noise of +-noise: residuals of a few bits under any predictor that
    follows a smooth signal, so that a Rice parameter chosen without regard to them costs little."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    out = np.zeros((n, nch), np.int64)
    for c in range(nch):
        out[:, c] = np.round(amp * np.sin(2 * np.pi * t * (0.003 + 0.002 * c))).astype(np.int64) + rng.integers(-noise, noise + 1, n)
    return out.astype(np.int32)


def near_fixed_coefs(order: int, precision: int = 12):
    """FIXED 2's predictor (2, -1) at shift precision - 3, with small taps of mixed sign behind it: every tap counts,
    and the prediction still follows a smooth signal."""
    shift = precision - 3
    cs = [2 << shift, -(1 << shift)] + [(-1) ** j * (1 + j % 3) for j in range(order - 2)]
    return cs[:order], shift


def alternating(n: int, bps: int) -> np.ndarray:
    """+max, -min, +max ... at bps bits."""
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    return np.where(np.arange(n) % 2 == 0, hi, lo).astype(np.int64)


def edge_catalogue():
    """Frames built around the limits at which K5 and K7 change path (a list of Edge).  Groups: a. partition orders 9,
    10 and 15 (K5 walks partitions in groups of 256); b. blocks on both sides of K5's residency limit; c. frames on
    both sides of the two staging limits; d. block sizes around K7's 64-sample hand-over and 128-sample ring, the
    smallest and the largest blocks, every table code; e. full scale at every sample width; f. LPC sums far beyond 32
    bits.  prop holds what a case was built for: frame_len (per frame, a list of (relation, bytes)), porder / psz /
    escapes (sub 0's partition order, partition size, escape partitions) and raw0 (one of them has raw width 0),
    resident, escape_raw (the raw width full scale needs), wasted, side_bits, wraps (some restored e + pred leaves
    int32), acc_over_32 (some prediction sum does), prec_shift, bs_code, sr_code."""
    out = []

    def add(group, name, pcm, subs, bps, prop, sr=44100, **kw):
        pcm = np.ascontiguousarray(pcm, np.int32)
        offs = []
        fr = frame(pcm, kw.pop("number", 0), bps, sr, subs, offsets=offs, **kw)
        out.append(Edge(group=group, name=name, pcm=pcm, frame=fr, frame_bytes=[len(fr)], blocks=[len(pcm)], bps=bps, rate=sr,
                        channels=pcm.shape[1], vbs=False, prop=prop, subs=subs, ch_code=kw.get("ch_code"), offsets=offs))

    # ---- a. partition groups: Rice parameters cycle per partition, escapes on both sides of the group boundary
    def grouped(porder, method=0):
        npart = 1 << porder
        esc = tuple(sorted({j for j in (0, K5_MAX_PARTS - 1, K5_MAX_PARTS, K5_MAX_PARTS + 1, npart - 1) if j < npart}))
        return dict(porder=porder, method=method, escape=esc, ks=[j % (31 if method else 15) for j in range(npart)])

    def silence_for(pcm, psz, order, part=K5_MAX_PARTS - 1):
        """zero residuals in one partition under any predictor: silence over it and the history it reads"""
        pcm[max(0, part * psz - order):(part + 1) * psz] = 0
        return pcm

    def prop_a(n, porder, **kw):
        return dict(porder=porder, psz=n >> porder, escapes=grouped(porder)["escape"], raw0=True, resident=n <= K5_RES_CAP, **kw)

    # (exactly one group: the walk's only trip ends at the last partition)
    add("a", "porder8_n2048_fixed1", silence_for(quiet_signal(2048, 1, 40), 8, 1), [dict(kind="fixed", order=1, **grouped(8))],
        16, prop_a(2048, 8))
    add("a", "porder9_n512_fixed1", silence_for(quiet_signal(512, 1, 41), 1, 1), [dict(kind="fixed", order=1, **grouped(9))],
        16, prop_a(512, 9))
    add("a", "porder9_n1024_fixed2", silence_for(quiet_signal(1024, 1, 42), 2, 2), [dict(kind="fixed", order=2, **grouped(9))],
        16, prop_a(1024, 9))
    c9, s9 = near_fixed_coefs(9)
    add("a", "porder9_n4608_lpc9", silence_for(quiet_signal(4608, 1, 43), 9, 9),
        [dict(kind="lpc", order=9, coefs=c9, precision=12, shift=s9, **grouped(9))], 16, prop_a(4608, 9))
    c10, s10 = near_fixed_coefs(10)
    add("a", "porder9_n5120_midside", silence_for(quiet_signal(5120, 2, 44, noise=1), 10, 10),
        [dict(kind="lpc", order=10, coefs=c10, precision=12, shift=s10, **grouped(9)),
         dict(kind="fixed", order=2, **grouped(9, method=1))], 16,
        prop_a(5120, 9, frame_len=[[(">", K5_FB_CAP), ("<=", K7_DFB_CAP)]]), ch_code=10)
    add("a", "porder10_n2048_rice2", silence_for(quiet_signal(2048, 1, 45), 2, 1),
        [dict(kind="fixed", order=1, **grouped(10, method=1))], 16, prop_a(2048, 10))
    for o in (0, 1):
        add("a", f"porder15_n32768_fixed{o}", silence_for(quiet_signal(32768, 1, 46 + o, amp=8), 1, o),
            [dict(kind="fixed", order=o, **grouped(15))], 16, prop_a(32768, 15))

    # ---- b. residency: the same forms in a resident block, one sample more, and a larger block with partitions
    for n, porder in ((K5_RES_CAP, 0), (K5_RES_CAP + 1, 0), (4640, 5)):
        esc = (0,) if porder == 0 else (0, 17, 31)
        pb = dict(resident=n <= K5_RES_CAP)
        x = test_signal(n, 2, 16, seed=50)
        mono = x[:, :1].copy()
        add("b", f"n{n}_fixed4", mono, [dict(kind="fixed", order=4, porder=porder)], 16, pb)
        c32, s32 = lpc_coefs(32, 15, seed=51)
        add("b", f"n{n}_lpc32_prec15", mono, [dict(kind="lpc", order=32, coefs=c32, precision=15, shift=s32, porder=porder)], 16, pb)
        add("b", f"n{n}_rice2", mono, [dict(kind="fixed", order=2, method=1, porder=porder)], 16, pb)
        add("b", f"n{n}_escape", mono, [dict(kind="fixed", order=1, porder=porder, escape=esc)], 16, dict(pb, escapes=esc))
        add("b", f"n{n}_wasted3", test_signal(n, 1, 16, seed=52, wasted=3), [dict(kind="fixed", order=2, wasted=3, porder=porder)],
            16, dict(pb, wasted=3))
        st = [dict(kind="fixed", order=2, porder=porder), dict(kind="fixed", order=1, porder=porder)]
        for cc in (8, 9, 10):
            add("b", f"n{n}_ch{cc}", x, st, 16, pb, ch_code=cc)
        y = test_signal(n, 8, 16, seed=53)
        y[:, 2] = -1234
        c8, s8 = lpc_coefs(8, 12, seed=54)
        subs = [dict(kind="lpc", order=8, coefs=c8, precision=12, shift=s8, porder=porder), dict(kind="fixed", order=1, porder=porder),
                dict(kind="constant"), dict(kind="fixed", order=2, method=1, porder=porder), dict(kind="verbatim"),
                dict(kind="fixed", order=3, porder=porder), dict(kind="fixed", order=0, porder=porder, escape=esc),
                dict(kind="fixed", order=4, porder=porder)]
        add("b", f"n{n}_eight_channels", y, subs, 16, pb)

    # ---- c. staging: frames of exactly cap and cap + 1 bytes (8-bit mono VERBATIM: n + 11 bytes), Rice-coded frames
    # just over each cap, and variable-block-size streams of cap, cap + 1 and a small frame
    rng = np.random.default_rng(60)
    noise8 = rng.integers(-128, 128, (2 * K7_DFB_CAP + 128, 1)).astype(np.int32)
    for cap in (K5_FB_CAP, K7_DFB_CAP):
        for extra in (0, 1):
            n = cap + extra - 11
            add("c", f"verbatim_{cap + extra}_bytes", noise8[:n], [dict(kind="verbatim")], 8, dict(frame_len=[[("==", cap + extra)]]))
    add("c", "rice_24bit_stereo_n8192", test_signal(8192, 2, 24, seed=61),
        [dict(kind="fixed", order=2, porder=6), dict(kind="fixed", order=1, porder=3)], 24,
        dict(frame_len=[[(">", K7_DFB_CAP)]]), ch_code=8)
    for cap in (K5_FB_CAP, K7_DFB_CAP):
        frames, first = [], 0
        sizes = [cap - 11, cap + 1 - 11 - (len(utf8(cap - 11)) - 1), 100]
        for k, n in enumerate(sizes):
            spec = dict(kind="verbatim") if k < 2 else dict(kind="fixed", order=1, porder=2)
            frames.append(frame(noise8[first:first + n], first, 8, 44100, [spec], vbs=True))
            first += n
        out.append(Edge(group="c", name=f"vbs_stream_{cap}", pcm=np.ascontiguousarray(noise8[:first]), frame=b"".join(frames),
                        frame_bytes=[len(f) for f in frames], blocks=sizes, bps=8, rate=44100, channels=1, vbs=True,
                        prop=dict(frame_len=[[("==", cap)], [("==", cap + 1)], [("<", 256)]]), subs=None, ch_code=None,
                        offsets=None))

    # ---- d. block sizes: a 32-tap history across K7's hand-over and ring, the largest blocks, the smallest
    c32, s32 = lpc_coefs(32, 12, seed=70)
    for n in (32, 33, K7_CHUNK - 1, K7_CHUNK, K7_CHUNK + 1, K7_RING - 1, K7_RING, K7_RING + 1, 16384):
        add("d", f"lpc32_n{n}", test_signal(n, 1, 16, seed=71), [dict(kind="lpc", order=32, coefs=c32, precision=12, shift=s32,
                                                                      porder=6 if n == 16384 else 0)], 16, dict(order=32))
    c32, s32 = lpc_coefs(32, 15, seed=72)
    add("d", "lpc32_n65535_24bit", test_signal(65535, 1, 24, seed=73),
        [dict(kind="lpc", order=32, coefs=c32, precision=15, shift=s32, porder=0)], 24, dict(order=32))
    for n in (1, 2, 3, 4):
        add("d", f"fixed{n}_n{n}", test_signal(16, 1, 16, seed=74)[:n] + 1000, [dict(kind="fixed", order=n, porder=0)], 16,
            dict(order=n))
    for n, code in sorted(BS_CODES.items(), key=lambda kv: kv[1]):
        add("d", f"constant_bs_code{code}", np.full((n, 1), -code, np.int32), [dict(kind="constant")], 16, dict(bs_code=code))
    for sr, code in sorted(SR_CODES.items(), key=lambda kv: kv[1]):
        add("d", f"constant_sr_code{code}", np.full((192, 1), code, np.int32), [dict(kind="constant")], 16, dict(sr_code=code), sr=sr)

    # ---- e. full scale at every width
    n = 80
    for bps in (4, 8, 12, 16, 17, 20, 24, 32):
        lo = -(1 << (bps - 1))
        alt = alternating(n, bps).reshape(-1, 1)
        add("e", f"bps{bps}_alt_verbatim", alt, [dict(kind="verbatim")], bps, {})
        # x[i] - 2 x[i-1] + x[i-2] = +-(2^(bps+1) - 2); at 32 bits that is +-2 after the wrap, and the prediction is
        # 3 * 2^31 away from the sample
        add("e", f"bps{bps}_alt_fixed2_rice2", alt, [dict(kind="fixed", order=2, method=1, porder=2, ks=[min(30, bps)] * 4)], bps,
            dict(wraps=True) if bps == 32 else {})
        # x[i] - x[i-1] = +-(2^bps - 1): bps + 1 bits as a signed field; at 32 bits -+1 after the wrap: 2 bits
        add("e", f"bps{bps}_alt_fixed1_escape", alt, [dict(kind="fixed", order=1, porder=1, escape=(0, 1))], bps,
            dict(escapes=(0, 1), escape_raw=2 if bps == 32 else bps + 1, **(dict(wraps=True) if bps == 32 else {})))
        add("e", f"bps{bps}_constant_min", np.full((n, 1), lo, np.int64), [dict(kind="constant")], bps, {})
        rng = np.random.default_rng(80 + bps)
        one = np.where(rng.integers(0, 2, (n, 1)) == 1, lo, 0)
        add("e", f"bps{bps}_one_bit_verbatim", one, [dict(kind="verbatim", wasted=bps - 1)], bps, dict(wasted=bps - 1))
        add("e", f"bps{bps}_one_bit_fixed1", one, [dict(kind="fixed", order=1, porder=0, wasted=bps - 1)], bps, dict(wasted=bps - 1))
        # stereo in anti-phase: the side takes bps + 1 bits.  At 32 bits |L - R| stays below 2^31 (the side of a
        # 32-bit stream is carried wrapped to int32): half scale, R = -L - 1, L - R = 2 L + 1
        if bps < 32:
            st = np.concatenate([alt, -alt - 1], axis=1)
        else:
            half = alternating(n, 31).reshape(-1, 1)
            st = np.concatenate([half, -half - 1], axis=1)
        for cc in (8, 9, 10):
            add("e", f"bps{bps}_antiphase_ch{cc}_verbatim", st, [dict(kind="verbatim"), dict(kind="verbatim")], bps,
                dict(side_bits=bps + 1), ch_code=cc)
            # (at 32 bits FIXED 1's residuals on half scale take 32 bits, one more than a raw field holds; FIXED 2's
            # are twice that and wrap to +-2)
            esc = dict(kind="fixed", order=2 if bps == 32 else 1, porder=0, escape=(0,))
            add("e", f"bps{bps}_antiphase_ch{cc}_escape", st, [esc, esc], bps, dict(side_bits=bps + 1), ch_code=cc)

    # ---- f. LPC arithmetic: 32 taps at the extremes of their precision, mixed in sign, on full-scale 24-bit noise; the
    # residuals are whatever 32 bits the wrap leaves, so RICE2 at parameter 30 keeps them to a few bits of unary
    rng = np.random.default_rng(90)
    noise24 = rng.integers(-(1 << 23), 1 << 23, (192, 1)).astype(np.int32)
    for prec, shift in ((1, 0), (2, 0), (5, 4), (15, 0), (15, 14), (15, 15)):
        cs = [-(1 << (prec - 1)) if j % 2 else (1 << (prec - 1)) - 1 for j in range(32)]
        if prec == 1:
            cs = [-1 if j % 3 else 0 for j in range(32)]
        add("f", f"lpc32_prec{prec}_shift{shift}", noise24,
            [dict(kind="lpc", order=32, coefs=cs, precision=prec, shift=shift, method=1, porder=0, ks=[30])], 24,
            dict(prec_shift=(prec, shift), acc_over_32=prec == 15, wraps=(prec, shift) == (15, 0)))
    return out


_EDGE_CASES = None


def edge_cases():
    """edge_catalogue(), generated once per process; the cases are shared and must not be changed."""
    global _EDGE_CASES
    if _EDGE_CASES is None:
        _EDGE_CASES = edge_catalogue()
        for e in _EDGE_CASES:
            e.pcm.setflags(write=False)
    return _EDGE_CASES
