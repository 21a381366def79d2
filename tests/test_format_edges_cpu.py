"""flacgen.edge_catalogue() on the CPU: every frame decodes back to its input through the test decoder
(oracle/flac_decode.c), and the property each case was built for -- the side of a kernel limit it lies on -- is read
back from the frame's bytes by a small parser of its own here, not taken from the generator's word.  A case whose
property does not hold fails."""
import numpy as np
import pytest

import flacgen
from flacgen import K5_FB_CAP, K5_MAX_PARTS, K5_RES_CAP, K7_CHUNK, K7_DFB_CAP, K7_RING

INT32 = (-(1 << 31), (1 << 31) - 1)
BS_OF_CODE = {v: k for k, v in flacgen.BS_CODES.items()}
REL = {"==": lambda a, b: a == b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b}


@pytest.fixture(scope="module")
def cat():
    return flacgen.edge_cases()


# ---- a frame parser: just enough of the format to say what a frame holds ------------------------------------

class Rd:
    def __init__(self, data: bytes):
        self.data = bytes(data)
        self.total = len(data) * 8
        bits = np.unpackbits(np.frombuffer(data, np.uint8))
        idx = np.where(bits == 1, np.arange(len(bits)), len(bits))
        self.next_one = np.minimum.accumulate(idx[::-1])[::-1].tolist()     # the first set bit at or behind p

    def u(self, p, nb):
        assert p + nb <= self.total
        if not nb:
            return 0
        b1 = (p + nb + 7) >> 3
        return (int.from_bytes(self.data[p >> 3:b1], "big") >> (b1 * 8 - p - nb)) & ((1 << nb) - 1)

    def s(self, p, nb):
        v = self.u(p, nb)
        return v - (1 << nb) if nb and v >> (nb - 1) else v


def parse_frame(data: bytes, channels: int, bps: int):
    """(header dict, subframes): per subframe type, order, wasted, precision, shift, coefs, method, porder, parts
    [(Rice parameter or None, raw width or None)], res (the residuals as written) and offsets (the bit at which each
    residual's codeword starts, and behind the last)."""
    r = Rd(data)
    assert r.u(0, 14) == 0x3FFE and r.u(14, 1) == 0
    h = dict(vbs=r.u(15, 1), bs_code=r.u(16, 4), sr_code=r.u(20, 4), ch_code=r.u(24, 4), bps_code=r.u(28, 3))
    b0 = r.u(32, 8)
    ones = 0
    while (b0 << ones) & 0x80:
        ones += 1
    p = 32 + 8 * max(ones, 1)
    if h["bs_code"] in (6, 7):
        nb = 8 if h["bs_code"] == 6 else 16
        n = r.u(p, nb) + 1
        p += nb
    else:
        n = BS_OF_CODE[h["bs_code"]]
    if h["sr_code"] >= 12:
        p += 8 if h["sr_code"] == 12 else 16
    p += 8                                                                  # CRC-8
    h["n"] = n
    subs = []
    for c in range(channels):
        cc = h["ch_code"]
        side = (cc == 8 and c == 1) or (cc == 9 and c == 0) or (cc == 10 and c == 1)
        assert r.u(p, 1) == 0
        code, wflag = r.u(p + 1, 6), r.u(p + 7, 1)
        p += 8
        wasted = 0
        if wflag:
            wasted = r.next_one[p] - p + 1
            p += wasted
        w = bps + (1 if side else 0) - wasted
        s = dict(wasted=wasted, w=w, order=0, parts=[], res=[], offsets=[])
        if code == 0:
            s["type"] = "constant"
            p += w
        elif code == 1:
            s["type"] = "verbatim"
            p += n * w
        else:
            s["type"], order = ("fixed", code - 8) if code < 32 else ("lpc", code - 31)
            s["order"] = order
            p += order * w
            if s["type"] == "lpc":
                prec, s["shift"] = r.u(p, 4) + 1, r.u(p + 4, 5)
                s["precision"] = prec
                p += 9
                s["coefs"] = [r.s(p + j * prec, prec) for j in range(order)]
                p += order * prec
            s["method"], s["porder"] = r.u(p, 2), r.u(p + 2, 4)
            p += 6
            pbits, esc = (5, 31) if s["method"] else (4, 15)
            psz = n >> s["porder"]
            for j in range(1 << s["porder"]):
                k = r.u(p, pbits)
                p += pbits
                cnt = psz - (order if j == 0 else 0)
                if k == esc:
                    raw = r.u(p, 5)
                    p += 5
                    s["parts"].append((None, raw))
                    for _ in range(cnt):
                        s["offsets"].append(p)
                        s["res"].append(r.s(p, raw))
                        p += raw
                else:
                    s["parts"].append((k, None))
                    for _ in range(cnt):
                        s["offsets"].append(p)
                        one = r.next_one[p]
                        u = ((one - p) << k) | r.u(one + 1, k)
                        p = one + 1 + k
                        s["res"].append((u >> 1) ^ -(u & 1))
            s["offsets"].append(p)
        subs.append(s)
    assert (p + 7) // 8 + 2 == len(data), "the frame does not end where its subframes do"
    return h, subs


def frames_of(e):
    off = 0
    for nb in e.frame_bytes:
        yield e.frame[off:off + nb]
        off += nb


@pytest.fixture(scope="module")
def parsed(cat):
    return {e.name: [parse_frame(f, e.channels, e.bps) for f in frames_of(e)] for e in cat}


# ---- the tests ---------------------------------------------------------------------------------------------

def test_names_are_unique_and_groups_complete(cat):
    assert len({e.name for e in cat}) == len(cat)
    assert {e.group for e in cat} == set("abcdef")


def test_oracle_decoder_returns_the_input(cat, decoder):
    for e in cat:
        got, sizes = decoder.decode(np.frombuffer(e.frame, np.uint8), e.channels, e.bps, e.n + 16)
        assert len(sizes) == len(e.frame_bytes), e
        assert got.shape == e.pcm.shape and np.array_equal(got, e.pcm), e


def test_recorded_offsets_are_where_the_codewords_are(cat, parsed):
    for e in cat:
        if e.offsets is None:
            continue
        h, subs = parsed[e.name][0]
        assert h["n"] == e.n and len(subs) == len(e.offsets) == e.channels
        for s, offs in zip(subs, e.offsets):
            assert offs == (s["offsets"] if s["type"] in ("fixed", "lpc") else []), e
            assert len(s["res"]) == (e.n - s["order"] if s["type"] in ("fixed", "lpc") else 0)


def leaves_int32(e, s, c=0):
    """(some restored e + pred leaves int32, some prediction sum does), computed as flacgen.residual() computes."""
    y = flacgen.channel_values(e.pcm, e.ch_code if e.ch_code is not None else e.channels - 1)[c] >> s["wasted"]
    acc, pred = flacgen.prediction(y, s["type"], s["order"], s.get("coefs"), s.get("shift", 0))
    total = np.array(s["res"], np.int64) + pred
    assert np.array_equal(((total + (1 << 31)) & 0xFFFFFFFF) - (1 << 31), y[s["order"]:])     # the wrap restores y
    return bool(np.any((total < INT32[0]) | (total > INT32[1]))), bool(np.any((acc < INT32[0]) | (acc > INT32[1])))


def test_each_case_has_the_property_it_was_built_for(cat, parsed):
    known = {"frame_len", "porder", "psz", "escapes", "raw0", "resident", "escape_raw", "wasted", "side_bits", "wraps",
             "acc_over_32", "prec_shift", "bs_code", "sr_code", "order"}
    for e in cat:
        pr = e.prop
        assert set(pr) <= known, e
        frames = parsed[e.name]
        h, subs = frames[0]
        s0 = subs[0]
        if "frame_len" in pr:
            assert len(pr["frame_len"]) == len(e.frame_bytes)
            for nb, rels in zip(e.frame_bytes, pr["frame_len"]):
                for rel, v in rels:
                    assert REL[rel](nb, v), (e, nb, rel, v)
        if "porder" in pr:
            assert s0["porder"] == pr["porder"] and len(s0["parts"]) == 1 << pr["porder"] and h["n"] >> s0["porder"] == pr["psz"]
        if "escapes" in pr:
            for s in subs:
                if s["type"] in ("fixed", "lpc") and (e.group != "b" or s is s0):
                    assert {j for j, (k, raw) in enumerate(s["parts"]) if raw is not None} == set(pr["escapes"]), e
        if pr.get("raw0"):
            assert any(raw == 0 for k, raw in s0["parts"]), e
        if "resident" in pr:
            assert (h["n"] <= K5_RES_CAP) == pr["resident"]
        if "escape_raw" in pr:
            assert [raw for k, raw in s0["parts"]] == [pr["escape_raw"]] * len(s0["parts"]), e
        if "wasted" in pr:
            assert s0["wasted"] == pr["wasted"] and s0["w"] == e.bps - pr["wasted"]
        if "side_bits" in pr:
            side = {8: 1, 9: 0, 10: 1}[h["ch_code"]]
            assert subs[side]["w"] == pr["side_bits"] == e.bps + 1
            l, r = e.pcm[:, 0].astype(np.int64), e.pcm[:, 1].astype(np.int64)
            if e.bps < 32:                                  # the side really needs the extra bit
                assert flacgen.minbits_signed([int(v) for v in l - r]) == e.bps + 1
            else:                                           # ... and at 32 bits stays inside int32, as the contract asks
                assert np.all(np.abs(l - r) < 1 << 31) and flacgen.minbits_signed([int(v) for v in l - r]) == 32
        if "wraps" in pr or "acc_over_32" in pr:
            wraps, over = leaves_int32(e, s0)
            assert wraps == pr.get("wraps", wraps) and over == pr.get("acc_over_32", over), (e, wraps, over)
        if "prec_shift" in pr:
            assert (s0["precision"], s0["shift"]) == pr["prec_shift"] and s0["order"] == 32
            lo, hi = -(1 << (s0["precision"] - 1)), (1 << (s0["precision"] - 1)) - 1
            assert set(s0["coefs"]) == {lo, hi} and s0["method"] == 1 and s0["parts"] == [(30, None)]
        if "bs_code" in pr:
            assert h["bs_code"] == pr["bs_code"]
        if "sr_code" in pr:
            assert h["sr_code"] == pr["sr_code"]
        if "order" in pr:
            assert s0["order"] == pr["order"] and s0["type"] == ("lpc" if pr["order"] == 32 else "fixed")


def test_group_a_crosses_the_partition_groups(cat, parsed):
    """More than one group of 256 partitions, neighbouring groups with different parameters, escapes on both sides of
    the first boundary and in the last partition."""
    names = set()
    for e in cat:
        if e.group != "a":
            continue
        names.add(e.name)
        for s in parsed[e.name][0][1]:
            parts = s["parts"]
            assert s["type"] in ("fixed", "lpc")
            mod = 31 if s["method"] else 15
            assert all(k == j % mod for j, (k, raw) in enumerate(parts) if k is not None)
            if e.name.startswith("porder8"):                       # exactly one group, an escape at each end of it
                assert len(parts) == K5_MAX_PARTS and parts[0][0] is None and parts[-1][0] is None
                continue
            assert len(parts) > K5_MAX_PARTS
            for j in (0, K5_MAX_PARTS - 1, K5_MAX_PARTS, K5_MAX_PARTS + 1, len(parts) - 1):
                assert parts[j][0] is None
            assert [p[0] for p in parts[1:K5_MAX_PARTS - 1]] != [p[0] for p in parts[K5_MAX_PARTS + 2:2 * K5_MAX_PARTS]]
    assert len(names) == 8
    by = {e.name: parsed[e.name][0] for e in cat if e.group == "a"}
    # the first partition is empty where the order is the partition size
    for name, order in (("porder9_n512_fixed1", 1), ("porder9_n1024_fixed2", 2), ("porder9_n4608_lpc9", 9)):
        h, subs = by[name]
        assert subs[0]["order"] == order == h["n"] >> subs[0]["porder"]
    h, subs = by["porder9_n5120_midside"]
    assert h["ch_code"] == 10 and [s["type"] for s in subs] == ["lpc", "fixed"] and [s["method"] for s in subs] == [0, 1]
    assert max(s["porder"] for name in by for s in by[name][1]) == 15


def test_every_limit_has_a_case_on_each_side(cat, parsed):
    sizes = {nb for e in cat for nb in e.frame_bytes}
    for cap in (K5_FB_CAP, K7_DFB_CAP):
        assert cap in sizes and cap + 1 in sizes
    ns = {e.n for e in cat}
    assert {K5_RES_CAP, K5_RES_CAP + 1, 4640} <= ns
    b = [e for e in cat if e.group == "b"]
    for form in ("fixed4", "lpc32_prec15", "rice2", "escape", "wasted3", "ch8", "ch9", "ch10", "eight_channels"):
        assert {e.n for e in b if e.name.endswith(form)} == {K5_RES_CAP, K5_RES_CAP + 1, 4640}
    for e in b:
        h, subs = parsed[e.name][0]
        types = [s["type"] for s in subs]
        if e.name.endswith("eight_channels"):
            assert "constant" in types and "verbatim" in types and len(subs) == 8
        if e.name.endswith("lpc32_prec15"):
            assert subs[0]["order"] == 32 and subs[0]["precision"] == 15
        if e.name.endswith("rice2"):
            assert subs[0]["method"] == 1
        if e.name.endswith("fixed4"):
            assert types == ["fixed"] and subs[0]["order"] == 4
    # Rice-coded frames over each staging cap, and one stream with both sides of it and a small frame
    assert any(e.frame_bytes[0] > K5_FB_CAP and parsed[e.name][0][1][0]["type"] == "lpc" for e in cat)
    assert any(e.frame_bytes[0] > K7_DFB_CAP and e.bps == 24 and e.channels == 2 and e.n == 8192 for e in cat)
    for cap in (K5_FB_CAP, K7_DFB_CAP):
        assert any(e.vbs and e.frame_bytes[:2] == [cap, cap + 1] and len(e.frame_bytes) == 3 for e in cat)
        for e in cat:
            if e.vbs:
                assert all(h["vbs"] == 1 for h, _ in parsed[e.name])
    # K7's hand-over and ring with a 32-tap history, the largest and the smallest blocks
    d32 = {e.n for e in cat if e.group == "d" and e.prop.get("order") == 32}
    assert d32 == {32, 33, K7_CHUNK - 1, K7_CHUNK, K7_CHUNK + 1, K7_RING - 1, K7_RING, K7_RING + 1, 16384, 65535}
    assert {1, 2, 3, 4, 32768} <= ns
    assert {e.prop["bs_code"] for e in cat if "bs_code" in e.prop} == {1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15}
    assert {e.prop["sr_code"] for e in cat if "sr_code" in e.prop} == set(range(1, 12))
    # every width, full scale in each
    for bps in (4, 8, 12, 16, 17, 20, 24, 32):
        grp = [e for e in cat if e.group == "e" and e.bps == bps]
        assert len(grp) == 12
        hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
        assert any(e.pcm.max() == hi and e.pcm.min() == lo for e in grp)
        assert any(e.prop.get("wasted") == bps - 1 for e in grp)
    assert {e.prop["prec_shift"] for e in cat if e.group == "f"} == {(1, 0), (2, 0), (5, 4), (15, 0), (15, 14), (15, 15)}


def test_existing_catalogues_are_unchanged():
    """catalogue() and utf8_catalogue() feed other tests: their frames are what they were (SHA-256 over all of them)."""
    import hashlib
    h = hashlib.sha256()
    for k in (16, 24):
        for c in flacgen.catalogue(bps=k):
            h.update(c[2])
    for c in flacgen.utf8_catalogue():
        h.update(c[2])
    assert h.hexdigest() == "f3951b689b8302a52b19f7aabc280cbdd0fd436a8ed75eff39918bf48957c527"


def test_the_limits_are_the_kernels():
    """The limits flacgen builds around are read from the kernels' sources: a kernel whose limit moves fails here."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def const(path, name, define=False):
        text = open(os.path.join(root, path)).read()
        pat = rf"#define\s+{name}\s+(\d+)" if define else rf"constexpr int {name} = (\d+);"
        found = re.findall(pat, text)
        assert len(found) == 1, (path, name)
        return int(found[0])

    assert const("include/flakehip.h", "FHIP_MAX_PARTS", define=True) == K5_MAX_PARTS
    assert const("flake_amd/csrc/k5_verify.hip", "RES_CAP") == K5_RES_CAP
    assert const("flake_amd/csrc/k5_verify.hip", "FB_CAP") == K5_FB_CAP
    assert const("flake_amd/csrc/k7_frame.h", "DFB_CAP") == K7_DFB_CAP
    assert const("flake_amd/csrc/k7_frame.h", "DT") == K7_CHUNK
    assert const("flake_amd/csrc/k7_frame.h", "RING") == K7_RING
