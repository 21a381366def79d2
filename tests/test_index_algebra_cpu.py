"""K8's algebra, in plain Python against flacgen.crc16: with P(p) the CRC-16 of s[0 .. p) and key(p) = P(p) x^(-8 p)
modulo x^16 + x^15 + x^2 + 1, two positions have equal keys iff the bytes between them have CRC-16 zero -- which, for a
span of two bytes and more, is "the CRC-16 of s[a .. q - 2) is what lies at q - 2", the frame's own check.  Also what
the kernel's way of computing the keys rests on: its constant for x^(-8), the order of x, and the XOR prefix sum of
per-chunk terms with the kernel's chunk sizes.  Runs without a GPU."""
import ctypes as C

import numpy as np

import flacgen
import flake_amd

POLY = 0x8005


def gf_mul(a, b):
    r = 0
    for i in range(15, -1, -1):
        r = ((r << 1) ^ POLY) & 0xFFFF if r & 0x8000 else (r << 1) & 0xFFFF
        if (b >> i) & 1:
            r ^= a
    return r


def gf_pow(b, e):
    r = 1
    while e:
        if e & 1:
            r = gf_mul(r, b)
        b = gf_mul(b, b)
        e >>= 1
    return r


def geometry():
    v = [C.c_int() for _ in range(4)]
    flake_amd.load_library().fhip_index_geometry(*[C.byref(x) for x in v])
    return [x.value for x in v]


def keys_by_definition(s, xinv8):
    """key(p) for p = 0 .. len(s), from the prefix CRCs themselves."""
    out, w = [], 1
    for p in range(len(s) + 1):
        out.append(gf_mul(flacgen.crc16(s[:p]), w))
        w = gf_mul(w, xinv8)
    return out


def planted(rng, n):
    """Random bytes in which some spans carry their own CRC-16 (nested and back to back), and a few zero bytes: both
    answers occur among the pairs."""
    s = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    for a, q in ((3, 40), (40, 41 + 30), (10, 90), (100, 102), (110, 113)):
        if q <= n:
            s[q - 2:q] = flacgen.crc16(bytes(s[a:q - 2])).to_bytes(2, "big")
    if n > 125:
        s[120:125] = bytes(5)
    return bytes(s)


def test_the_kernels_constant_is_x_to_the_minus_8():
    lane, wg, end_lane, xinv8 = geometry()
    assert gf_mul(xinv8, 0x100) == 1                    # x^8 is 0x100
    assert xinv8 == gf_pow(2, 32767 - 8)
    assert gf_pow(2, 32767) == 1 and all(gf_pow(2, 32767 // f) != 1 for f in (7, 31, 151))     # the order of x is 32767
    assert wg % lane == 0 and wg % end_lane == 0 and lane >= 1


def test_equal_keys_iff_the_span_checks_out():
    _, _, _, xinv8 = geometry()
    rng = np.random.default_rng(5)
    yes = no = 0
    for trial in range(4):
        s = planted(rng, 160)
        key = keys_by_definition(s, xinv8)
        pos = sorted(set([0, 1, 2, 3, 10, 40, 41, 42, 71, 90, 100, 101, 102, 110, 113, 120, 121, 122, 123, 124, 125, 160] +
                         [int(v) for v in rng.integers(0, 161, 16)]))
        assert len(pos) >= 30
        for i, a in enumerate(pos):
            for q in pos[i:]:
                zero = flacgen.crc16(s[a:q]) == 0
                assert (key[a] == key[q]) == zero, (trial, a, q)
                if q - a >= 2:          # the frame's own check (lengths 0 and 1 have no two bytes to compare with)
                    assert zero == (flacgen.crc16(s[a:q - 2]) == int.from_bytes(s[q - 2:q], "big")), (trial, a, q)
                yes += zero
                no += not zero
    assert yes > 40 and no > 1000


def test_keys_as_an_xor_prefix_of_chunk_terms():
    """What the candidate pass does: a lane's term is crc(its bytes) x^(-8 (offset of their end in the workgroup)), a
    workgroup's the XOR of its lanes' times x^(-8 base) with the exponent taken modulo the order of x; key(p) is the
    XOR of everything before p.  Held against the definition at every position of a stream that spans three
    workgroups and ends inside a lane."""
    lane, wg, _, xinv8 = geometry()
    rng = np.random.default_rng(9)
    s = rng.integers(0, 256, 2 * wg + 5 * lane + 3, dtype=np.uint8).tobytes()
    want = keys_by_definition(s, xinv8)
    xinv = [1]
    for _ in range(wg):
        xinv.append(gf_mul(xinv[-1], xinv8))
    got = [0] * (len(s) + 1)
    key_wg = 0
    for base in range(0, len(s), wg):
        e8 = (base % 32767) * 8 % 32767
        wpow = gf_pow(2, 32767 - e8 if e8 else 0)
        assert wpow == gf_pow(xinv8, base)
        local = 0
        for o in range(0, min(wg, len(s) - base), lane):
            chunk = s[base + o:base + o + lane]
            for j in range(len(chunk) + 1):
                got[base + o + j] = key_wg ^ gf_mul(wpow, local ^ gf_mul(flacgen.crc16(chunk[:j]), xinv[o + j]))
            local ^= gf_mul(flacgen.crc16(chunk), xinv[o + len(chunk)])
        key_wg ^= gf_mul(wpow, local)
    assert got == want
