"""A small pure-Python FLAC frame writer for the verifier's tests.

It writes frames in forms this project's encoder never emits -- every subframe type, FIXED 0-4 and
LPC 1-32, wasted bits, RICE and RICE2, escape partitions (raw width 0 included), every channel
assignment, explicit block-size and sample-rate codes, long UTF-8 numbers -- straight from the FLAC
format.  Samples are restored the way libFLAC does (64-bit prediction sum, arithmetic shift, int32
wrap), so the residual written here is the one a decoder needs.
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
        v &= (1 << nb) - 1 if nb else 0
        self.bits.extend((v >> (nb - 1 - i)) & 1 for i in range(nb))

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


def residual(y: np.ndarray, kind: str, order: int, coefs=None, shift: int = 0) -> list[int]:
    """e[i] for i >= order, int32-wrapped as a decoder restores them."""
    y = [int(v) for v in y]
    cs = FIXED_COEFS[order] if kind == "fixed" else list(coefs)
    out = []
    for i in range(order, len(y)):
        acc = sum(c * y[i - 1 - j] for j, c in enumerate(cs))
        pred = acc if kind == "fixed" else acc >> shift
        e = (y[i] - pred) & 0xFFFFFFFF
        out.append(e - (1 << 32) if e >= 1 << 31 else e)
    return out


def minbits_signed(vals) -> int:
    m = 0
    for v in vals:
        b = (v.bit_length() + 1) if v >= 0 else ((-v - 1).bit_length() + 1)
        m = max(m, b if v != 0 else 0)
    return m


def put_residual(w: BitWriter, res: list[int], n: int, order: int, method: int, porder: int,
                 escape=(), ks=None) -> None:
    """escape: partitions written raw ("escape partitions"); ks: Rice parameter per partition (None: a
    simple estimate)."""
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
            w.put(pbits, esc)
            w.put(5, raw)
            for e in part:
                w.put(raw, e)
            continue
        if ks is not None:
            k = ks[j]
        else:
            mean = sum(zigzag(e) for e in part) / max(1, len(part))
            k = max(0, int(mean).bit_length() - 1)
        k = min(k, esc - 1)
        w.put(pbits, k)
        for e in part:
            u = zigzag(e)
            w.unary(u >> k)
            w.put(k, u & ((1 << k) - 1))


def put_subframe(w: BitWriter, y: np.ndarray, bps: int, spec: dict) -> None:
    """spec: kind (constant | verbatim | fixed | lpc), order, coefs, precision, shift, wasted, method,
    porder, escape, ks."""
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
                 spec.get("ks"))


def frame(pcm: np.ndarray, number: int, bps: int, sample_rate: int, subframes: list[dict], ch_code=None,
          vbs: bool = False, bs_code=None, sr_code=None, bps_code=None) -> bytes:
    """One frame of pcm ([n][channels] int32).  number: the frame number (fixed blocks) or the first sample
    (vbs).  bs_code / sr_code / bps_code: force a header code (6 / 7, 12 / 13 / 14 carry the value)."""
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
        put_subframe(w, vals[c], bps + (1 if side else 0), spec)
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
