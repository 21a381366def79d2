"""K8, frame discovery on the device (fhip_index_frames, fhip_index_frames_dev, flake_amd_decode_index,
flake_amd_decode_set_index, the CLI): the contract is the CPU indexer's answer, exactly, so every case here runs
flake_amd.index_frames on the same bytes and compares sizes, count, consumed and the -1 answers with it -- no expected
value is typed by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd
import flacgen
import goldenlib as G
from test_decode_index_cpu import SUB, fixed_stream, streaminfo, vbs_stream

pytestmark = pytest.mark.gpu

V = flake_amd
SENT = -1234567
GUARD = 32
CLI = os.path.join(V.LIB_DIR, "flake_amd_cli")


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(scope="module")
def handles():
    """One handle per format (channels, bits per sample, rate): K8 reads nothing else of it."""
    made = {}

    def get(si):
        key = (int(si.channels), int(si.bits_per_sample), int(si.sample_rate))
        if key not in made:
            made[key] = V.Encoder(V.level_params(5, channels=key[0], bits_per_sample=key[1], sample_rate=key[2]), max_frames=4)
        return made[key]
    yield get
    for enc in made.values():
        enc.close()


def geometry():
    v = [C.c_int() for _ in range(4)]
    V.load_library().fhip_index_geometry(*[C.byref(x) for x in v])
    return [x.value for x in v]


def cpu_ranges(si, stream, first, frame_cap):
    """The contract: for r in ranges: flake_amd_index_frames(range r, cap = frame_cap - frames so far)."""
    stream = bytes(stream)
    sizes, frames, cons, var = [], [], [], []
    for r in range(len(first) - 1):
        piece = stream[first[r]:first[r + 1]]
        got = V.index_frames(si, piece, cap=frame_cap - len(sizes))
        begins = V.index_frames(si, piece, cap=1) is not None and len(piece) > 0
        var.append(piece[1] & 1 if begins else 0)
        if got is None:
            frames.append(-1)
            cons.append(0)
        else:
            sizes += [int(v) for v in got[0]]
            frames.append(len(got[0]))
            cons.append(got[1])
    return sizes, frames, cons, var


def device_ranges(enc, si, stream, first, frame_cap):
    """fhip_index_frames with sentinels around every output; returns what cpu_ranges returns."""
    st = np.frombuffer(bytes(stream), dtype=np.uint8)
    rf = np.asarray(first, dtype=np.int64)
    nr = len(rf) - 1
    fb = np.full(frame_cap + 2 * GUARD, SENT, np.int32)
    r_frames, r_var = np.full(nr + 2 * GUARD, SENT, np.int32), np.full(nr + 2 * GUARD, SENT, np.int32)
    r_cons = np.full(nr + 2 * GUARD, SENT, np.int64)
    ii = V.IndexIn(st.ctypes.data if st.size else None, st.size, rf.ctypes.data, nr, int(si.max_block_size), frame_cap)
    io = V.IndexOut(fb[GUARD:].ctypes.data, r_frames[GUARD:].ctypes.data, r_cons[GUARD:].ctypes.data, r_var[GUARD:].ctypes.data)
    rc = enc.lib.fhip_index_frames(enc._h, C.byref(ii), C.byref(io))
    assert rc == V.OK, enc.lib.fhip_last_error(enc._h)
    for a in (r_frames, r_var, r_cons):
        assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + nr:] == SENT)
    frames = [int(v) for v in r_frames[GUARD:GUARD + nr]]
    total = sum(f for f in frames if f > 0)
    assert total <= frame_cap
    assert np.all(fb[:GUARD] == SENT) and np.all(fb[GUARD + total:] == SENT)       # nothing behind the last frame is written
    return ([int(v) for v in fb[GUARD:GUARD + total]], frames, [int(v) for v in r_cons[GUARD:GUARD + nr]],
            [int(v) for v in r_var[GUARD:GUARD + nr]])


def agree(handles, si, stream, first=None, frame_cap=None):
    stream = bytes(stream)
    first = [0, len(stream)] if first is None else list(first)
    if frame_cap is None:
        frame_cap = len(stream) // 8 + len(first)
    want = cpu_ranges(si, stream, first, frame_cap)
    got = device_ranges(handles(si), si, stream, first, frame_cap)
    assert got[1] == want[1], ("frames", got[1], want[1])
    assert got[2] == want[2], ("consumed", got[2], want[2])
    assert got[0] == want[0], "sizes"
    assert got[3] == want[3], ("variable", got[3], want[3])
    return want


# ---- the streams of tests/test_decode_index_cpu.py ------------------------------------------------------

def decoy_streams():
    """(the stream with a complete valid header, expected number and all, inside a VERBATIM subframe; the same bytes
    made a real boundary), as test_index_skips_a_decoy_header builds them."""
    n, bps = 192, 16
    good_next = flacgen.frame(flacgen.test_signal(n, 1, bps, seed=5), 4, bps, 44100, SUB)
    hdr = good_next[:6]
    x = flacgen.test_signal(n, 1, bps, seed=6)
    for k in range(3):
        v = (hdr[2 * k] << 8) | hdr[2 * k + 1]
        x[10 + k, 0] = v - (1 << 16) if v >= 1 << 15 else v
    decoy = flacgen.frame(x, 3, bps, 44100, [dict(kind="verbatim")])
    at = decoy.find(hdr)
    assert at > 6
    before, _ = fixed_stream([n] * 3, first=0)
    body = decoy[:at - 2]
    split = body + flacgen.crc16(body).to_bytes(2, "big")
    return b"".join(before + [decoy, good_next]), b"".join(before) + split + decoy[at:]


def test_fixed_blocks_short_last_frame_and_caps(handles):
    frames, _ = fixed_stream([1152] * 5 + [200], first=7)
    si = streaminfo(channels=1, max_block=1152)
    want = agree(handles, si, b"".join(frames))
    assert want[1] == [6]
    for cap in (0, 3, 100):
        agree(handles, si, b"".join(frames), frame_cap=cap)
    agree(handles, si, b"")                                     # the empty stream


def test_variable_blocks_long_numbers(handles):
    frames = vbs_stream([256, 1000, 192, 17], first=(1 << 31) - 300)          # six- and seven-byte numbers
    want = agree(handles, streaminfo(channels=1, max_block=4096, min_block=16), b"".join(frames))
    assert want[1] == [4] and want[3] == [1]


def test_decoy_header_and_the_same_bytes_as_a_boundary(handles):
    si = streaminfo(channels=1, max_block=192)
    a, b = decoy_streams()
    assert agree(handles, si, a)[1] == [5]
    assert agree(handles, si, b)[1][0] >= 4                     # the three frames in front, then the split one


def test_cut_and_corrupted_last_frame(handles):
    frames, _ = fixed_stream([1152] * 4, first=0)
    si = streaminfo(channels=1, max_block=1152)
    stream = b"".join(frames)
    assert agree(handles, si, stream[:len(stream) - len(frames[-1]) // 2])[1] == [3]
    bad = bytearray(stream)
    bad[-20] ^= 0x10
    assert agree(handles, si, bad)[1] == [3]


def test_garbage_first(handles):
    frames, _ = fixed_stream([192] * 2)
    si = streaminfo(channels=1, max_block=192)
    assert agree(handles, si, b"\x00\x01\x02" + b"".join(frames))[1] == [-1]
    assert agree(handles, si, b"\xff\xf8" + bytes(40))[1] == [-1]
    assert agree(handles, streaminfo(channels=2, max_block=192), b"".join(frames))[1] == [-1]


def test_numbering_break(handles):
    a, _ = fixed_stream([192] * 2, first=0)
    b, _ = fixed_stream([192] * 2, first=9, seed=4)
    si = streaminfo(channels=1, max_block=192)
    want = agree(handles, si, b"".join(a + b))
    assert want[1] == [2] and want[2] == [len(b"".join(a + b))]      # the rest as one span that ends at `bytes`
    assert agree(handles, si, b"".join(a + b)[:-5])[1] == [1]


def test_golden_reference_streams(handles):
    z = G.load("ref_path.npz")
    seen = 0
    for key in z.keys():
        if not key.startswith("frames_"):
            continue
        name = key[len("frames_"):]
        p = V.Params(*[int(v) for v in z["params_" + name]])
        if p.allow_vbs:
            continue
        si = streaminfo(channels=p.channels, bps=p.bits_per_sample, rate=p.sample_rate, max_block=p.block_size)
        want = agree(handles, si, z[key].tobytes())
        assert want[1] == [len(z["framelens_" + name])], name
        seen += 1
    assert seen >= 3


# ---- chunk boundaries --------------------------------------------------------------------------------

def small_frames(count, first=0, seed=0, vbs=False):
    """Mono frames of 16 samples whose lengths vary (the noise decides the Rice parameter and the escape)."""
    out = []
    for i in range(count):
        x = flacgen.test_signal(16, 1, 16, seed=seed + i)
        x = (x.astype(np.int64) * (1 + i % 5) // 5).astype(np.int32)
        spec = [dict(kind="verbatim")] if i % 7 == 3 else SUB
        out.append(flacgen.frame(x, first + (16 * i if vbs else i), 16, 44100, spec, vbs=vbs))
    return out


@pytest.fixture(scope="module")
def small300():
    return small_frames(300)


def test_every_residue_of_both_chunks(handles, small300):
    """A range of filler in front shifts the whole stream a byte at a time: every frame start and every header byte
    falls on every residue of the candidate pass's lane chunk (which takes the CRC prefixes too), the stream's end on
    every residue of the end pass's lane chunk, and one header walks across a workgroup boundary byte by byte."""
    lane, wg, end_lane, _ = geometry()
    si = streaminfo(channels=1, max_block=16)
    stream = b"".join(small300)
    assert len(stream) > 2 * wg and len({len(f) for f in small300}) > 4
    starts = np.concatenate([[0], np.cumsum([len(f) for f in small300])])
    near = int(starts[np.searchsorted(starts, wg)])             # the first frame start at or behind the boundary
    shifts = set(range(max(lane, end_lane) + 1))
    shifts |= {s for s in range(2 * wg) if -8 <= (near + s) % wg - wg <= 0 or (near + s) % wg <= 1}
    assert len(shifts) < 120
    want0 = agree(handles, si, stream)
    assert want0[1] == [300]
    for s in sorted(shifts):
        filler = bytes([0x55]) * s
        want = agree(handles, si, filler + stream, first=[0, s, s + len(stream)])
        assert want[1] == ([-1] if s else [0]) + [300] and want[0] == want0[0], s


def test_more_frames_than_any_one_trip(handles):
    """3000 frames in about 120 KB: dozens of scan workgroups, far more candidates than the walk takes in a trip, and
    as 300 ranges of ten frames more ranges than the range pass takes in one."""
    frames = small_frames(3000, first=5)
    si = streaminfo(channels=1, max_block=16)
    stream = b"".join(frames)
    assert agree(handles, si, stream)[1] == [3000]
    first = [0] + [int(v) for v in np.cumsum([sum(len(f) for f in frames[k:k + 10]) for k in range(0, 3000, 10)])]
    want = agree(handles, si, stream, first=first)
    assert want[1] == [10] * 300
    agree(handles, si, stream, first=first, frame_cap=2995)     # the cap falls inside the last range


def test_a_stream_of_more_workgroups_than_one_scan_trip(handles):
    """Over a mebibyte: the scan over the candidate pass's workgroups carries from one trip to the next."""
    _, wg, _, _ = geometry()
    nf = 24
    with V.HostEncoder(level=5, bits_per_sample=16) as he:
        n = he.ctx.params.block_size
        stream, _ = he.encode_frames(V.synth_pcm(nf, n, 2, 16).reshape(-1, 2), n, 0)
        si, _ = V.read_streaminfo(V.write_streaminfo(he.streaminfo()))
    stream = bytes(stream)
    if len(stream) <= 257 * wg:                                 # (a quiet signal: repeat the stream as ranges instead)
        reps = 257 * wg // len(stream) + 1
        first = [k * len(stream) for k in range(reps + 1)]
        want = agree(handles, si, stream * reps, first=first)
        assert want[1] == [nf] * reps
    else:
        assert agree(handles, si, stream)[1] == [nf]


# ---- false syncs -------------------------------------------------------------------------------------

def test_dense_false_syncs_and_a_false_header_whose_key_differs(handles):
    """VERBATIM payloads of FF F8 repeated: thousands of sync hits, four real headers.  In the second frame three
    samples spell the complete header the next frame begins with -- sync, codes, the expected number, CRC-8 -- so that
    candidate passes everything but the CRC-16 of the span in front of it."""
    n = 1024
    nxt = flacgen.frame(np.full((n, 1), -8, np.int32), 2, 16, 44100, [dict(kind="verbatim")])
    hdr = nxt[:flacgen_header_len(nxt)]
    frames = []
    for i in range(4):
        x = np.full((n, 1), -8, np.int32)                       # 0xFFF8
        if i == 1:
            assert len(hdr) % 2 == 0
            for k in range(len(hdr) // 2):
                v = (hdr[2 * k] << 8) | hdr[2 * k + 1]
                x[100 + k, 0] = v - (1 << 16) if v >= 1 << 15 else v
        frames.append(flacgen.frame(x, i, 16, 44100, [dict(kind="verbatim")]))
    assert frames[2] == nxt and frames[1].find(hdr) > 8
    stream = b"".join(frames)
    assert stream.count(b"\xff\xf8") > 3500
    si = streaminfo(channels=1, max_block=n)
    assert V.index_frames(si, frames[1][frames[1].find(hdr):] + frames[2] + frames[3]) is not None    # it IS a header
    want = agree(handles, si, stream)
    assert want[1] == [4] and want[0] == [len(f) for f in frames]


def flacgen_header_len(frame):
    """The header's length: the first prefix whose CRC-8 is the byte behind it (6 .. 16 bytes)."""
    for k in range(5, 16):
        if flacgen.crc8(frame[:k]) == frame[k]:
            return k + 1
    raise AssertionError("no header")


# ---- the header predicate, compiled for the device ---------------------------------------------------

def test_header_catalogue_a_range_per_case(handles):
    """The header catalogue of tests/test_flac_header_cpu.py laid end to end, each case a range of its own that ends at
    the case's `avail`: K8 answers -1 where the range does not begin with a header and 0 where it does (a header alone
    closes no frame), so range_frames against the CPU indexer's is the predicate's verdict from both compilers.  One
    format, one call: every valid header, every truncation of those whose strategy bit is 0, every bit flip of the two
    longest of them and the reserved and disagreeing codes."""
    import test_flac_header_cpu as H
    valid = H.valid_headers()
    fixed = [h for h in valid if not h[1] & 1]
    pieces = list(valid)
    pieces += [h[:avail] for h in fixed for avail in range(1, len(h))]
    for h in sorted(fixed, key=len)[-2:]:
        for bit in range(8 * len(h)):
            x = bytearray(h)
            x[bit >> 3] ^= 0x80 >> (bit & 7)
            pieces.append(bytes(x))
    pieces += [h for fmt, h, _ in H.field_cases() if fmt == H.BASE]
    assert 300 <= len(pieces) <= 800 and max(map(len, pieces)) == 16
    si = streaminfo(channels=H.BASE[0], bps=H.BASE[1], rate=H.BASE[2], max_block=H.BASE[3])
    first = [0] + [int(v) for v in np.cumsum([len(p) for p in pieces])]
    want = agree(handles, si, b"".join(pieces), first=first)
    assert want[0] == [] and want[1].count(0) >= 40 and want[1].count(-1) >= 40
    assert want[1] == [0 if H.reference(H.BASE, p, len(p)) else -1 for p in pieces]


# ---- many ranges -------------------------------------------------------------------------------------

def test_eight_ranges_one_call(handles):
    si = streaminfo(channels=1, max_block=4096, min_block=16)
    a, _ = fixed_stream([192] * 6 + [50], first=3)
    b = vbs_stream([256, 1000, 192, 17, 640], first=1 << 20)
    c, _ = fixed_stream([1152] * 3, first=0, seed=8)
    d, _ = fixed_stream([576] * 5, first=200, seed=9)
    e, _ = fixed_stream([16] * 9, first=0, seed=10)
    parts = [b"".join(a), b"".join(b), b"", b"\x12\x34" + b"".join(c), b"".join(d), b"".join(c)[:-7], b"".join(e),
             b"".join(vbs_stream([4096, 100], first=0, seed=3))]
    first = [0] + [int(v) for v in np.cumsum([len(p) for p in parts])]
    stream = b"".join(parts)
    want = agree(handles, si, stream, first=first)
    assert want[1] == [7, 5, 0, -1, 5, 2, 9, 2] and want[3] == [0, 1, 0, 0, 0, 0, 0, 1]
    cut = agree(handles, si, stream, first=first, frame_cap=7 + 5 + 3)        # inside the fifth range
    assert cut[1] == [7, 5, 0, -1, 3, 0, 0, 0]
    agree(handles, si, stream, first=first, frame_cap=0)


# ---- seeded corruption -------------------------------------------------------------------------------

def test_seeded_corruption(handles):
    frames, _ = fixed_stream([192] * 40, first=0)
    si = streaminfo(channels=1, max_block=192)
    good = b"".join(frames)
    counts = set()
    for seed in range(64):
        rng = np.random.default_rng(1000 + seed)
        bad = bytearray(good)
        bad[int(rng.integers(0, len(bad)))] ^= int(rng.integers(1, 256))
        counts.add(agree(handles, si, bad)[1][0])
    for seed in range(16):
        rng = np.random.default_rng(2000 + seed)
        at, k = int(rng.integers(0, len(good))), int(rng.integers(1, 9))
        bad = good[:at] + good[at + k:] if seed % 2 else good[:at] + rng.integers(0, 256, k, dtype=np.uint8).tobytes() + good[at:]
        counts.add(agree(handles, si, bad)[1][0])
    assert len(counts) > 10                                     # the damage landed in many different frames


# ---- the device entry --------------------------------------------------------------------------------

def test_device_entry(torch, handles, small300):
    si = streaminfo(channels=1, max_block=16)
    enc = handles(si)
    stream = b"".join(small300)
    half = sum(len(f) for f in small300[:150])
    dev = torch.device("cuda")
    names = ["k_index_scan<false>", "k_index_wgscan", "k_index_scan<true>", "k_index_walk", "k_index_ranges", "k_index_emit"]

    def run(dstream, nbytes, first, cap):
        nr = len(first) - 1
        drf = torch.tensor(first, dtype=torch.int64, device=dev)
        dfb = torch.full((cap + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        dfr = torch.full((nr + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        dva = torch.full((nr + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        dco = torch.full((nr + 2 * GUARD,), SENT, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        enc.index_ranges_dev(dstream, nbytes, drf, nr, si.max_block_size, cap, dfb[GUARD:], dfr[GUARD:], dco[GUARD:], dva[GUARD:])
        assert enc.last_launches() == names
        enc.sync()
        fb, fr, va, co = dfb.cpu().numpy(), dfr.cpu().numpy(), dva.cpu().numpy(), dco.cpu().numpy()
        frames = [int(v) for v in fr[GUARD:GUARD + nr]]
        total = sum(f for f in frames if f > 0)
        for a in (fr, va, co):
            assert np.all(a[:GUARD] == SENT) and np.all(a[GUARD + nr:] == SENT)
        assert np.all(fb[:GUARD] == SENT) and np.all(fb[GUARD + total:] == SENT)
        return ([int(v) for v in fb[GUARD:GUARD + total]], frames, [int(v) for v in co[GUARD:GUARD + nr]],
                [int(v) for v in va[GUARD:GUARD + nr]])

    # the stream fills its allocation to the last byte; device-resident inputs give the host entry's result
    ds = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dev)
    first = [0, half, len(stream)]
    assert run(ds, len(stream), first, 400) == cpu_ranges(si, stream, first, 400)
    # offsets beyond stream_bytes (and one below 0) read nothing outside the buffer: the answer is that of the
    # offsets clamped into the stream
    wild = [-5, half, len(stream) + 1000, len(stream) + (1 << 40)]
    clamped = [0, half, len(stream), len(stream)]
    assert run(ds, len(stream), wild, 400) == cpu_ranges(si, stream, clamped, 400)
    # a stream that does not start on a 16-byte boundary and ends with its allocation
    cut = small300[0][:3]
    odd = torch.from_numpy(np.frombuffer(cut + stream, dtype=np.uint8).copy()).to(dev)
    assert run(odd[3:], len(stream), [0, len(stream)], 400) == cpu_ranges(si, stream, [0, len(stream)], 400)
    # an empty stream: no scan launches at all
    drf = torch.zeros(2, dtype=torch.int64, device=dev)
    out = [torch.full((4,), SENT, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.int64, torch.int32)]
    enc.index_ranges_dev(ds, 0, drf, 1, 16, 4, out[0], out[1], out[2], out[3])
    assert enc.last_launches() == [n for n in names if "scan<" not in n]
    enc.sync()
    assert [int(o.cpu()[0]) for o in out] == [SENT, 0, 0, 0]


def test_refusals_queue_nothing(handles):
    si = streaminfo(channels=1, max_block=192)
    enc = handles(si)
    frames, _ = fixed_stream([192] * 2)
    stream = b"".join(frames)
    assert enc.index_ranges(stream, [0, len(stream)])[0] == V.OK and enc.last_launches()
    for first in ([1, len(stream)], [0, 50, 40, len(stream)], [0, len(stream) - 1], [0]):
        rc = enc.index_ranges(stream, first)[0]
        assert rc == V.E_INVALID and enc.last_launches() == [], first
    assert enc.index_ranges(stream, [0, len(stream)], frame_cap=-1)[0] == V.E_INVALID
    assert enc.index_ranges(stream, [0, len(stream)], max_block_size=-1)[0] == V.E_INVALID
    ii = V.IndexIn(None, 1 << 31, None, 1, 0, 4)
    assert enc.lib.fhip_index_frames(enc._h, C.byref(ii), None) == V.E_INVALID
    rf = np.asarray([0, 1 << 31], np.int64)
    out = np.zeros(8, np.int64)
    ii = V.IndexIn(out.ctypes.data, 1 << 31, rf.ctypes.data, 1, 0, 4)
    io = V.IndexOut(out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data)
    assert enc.lib.fhip_index_frames(enc._h, C.byref(ii), C.byref(io)) == V.E_INVALID       # 2 GiB: refused unread
    assert enc.lib.fhip_index_frames_dev(enc._h, C.byref(ii), C.byref(io)) == V.E_INVALID and enc.last_launches() == []


def test_profiling_names_every_launch(handles):
    si = streaminfo(channels=1, max_block=192)
    enc = handles(si)
    frames, _ = fixed_stream([192] * 2)
    enc.set_profiling(True)
    try:
        enc.kernel_times(reset=True)
        assert enc.index_ranges(b"".join(frames), [0, sum(len(f) for f in frames)])[0] == V.OK
        enc.sync()
        kt = enc.kernel_times(reset=True)
    finally:
        enc.set_profiling(False)
    for name in ("k_index_count", "k_index_wgscan", "k_index_scatter", "k_index_walk", "k_index_ranges", "k_index_emit"):
        assert kt[name][1] == 1 and kt[name][0] > 0, (name, kt)
    assert kt["k_decode"][1] == 0


# ---- end to end ----------------------------------------------------------------------------------------

def test_host_decoder_index_feeds_decode_frames():
    from test_gpu_decode_host import encode_stream
    for level, tail in ((5, 1000), (10, 0)):
        n, pcm, stream, si = encode_stream(level, 16, 6, tail, seed=level)
        with V.HostDecoder(si) as d:
            got = d.index(stream)
            want = V.index_frames(si, stream)
            assert got is not None and list(got[0]) == list(want[0]) and got[1] == want[1] == len(stream)
            few = d.index(stream, cap=2)
            assert list(few[0]) == list(want[0][:2]) and few[1] == int(want[0][:2].sum())
            assert d.index(b"\x00" + bytes(stream)) is None
            out = d.decode_frames(stream, got[0], len(pcm), 2)
            assert np.array_equal(out, pcm.astype(np.int16))
            assert d.md5() == bytes(si.md5sum) != bytes(16)


@pytest.fixture(scope="module")
def four_files():
    from test_gpu_decode_set import encode_set
    return encode_set([64 * 6 + 10, 64 * 3, 64 * 9 + 63, 200], 64, 5, 0, 300)


def test_decode_set_index_feeds_decode_runs(four_files):
    like = V.HostStreaminfo(min_block_size=16, max_block_size=64, sample_rate=44100, channels=2, bits_per_sample=16)
    with V.DecodeSet(like, 4) as g:
        found = g.index([x["frames"] for x in four_files])
        for x, got in zip(four_files, found):
            want = V.index_frames(like, x["frames"])
            assert got is not None and list(got[0]) == list(want[0]) == list(x["sizes"]) and got[1] == want[1]
        outs = g.decode_runs([(s, x["frames"], found[s][0]) for s, x in enumerate(four_files)],
                             sum(len(x["pcm"]) for x in four_files), 2)
        for s, x in enumerate(four_files):
            assert np.array_equal(outs[s], x["pcm"].astype(np.int16)), s
            assert g.md5(s) == bytes(x["si"].md5sum) != bytes(16)
        # a refused file among good ones takes no room
        mixed = g.index([four_files[0]["frames"], b"\x01\x02\x03", four_files[3]["frames"][:-3]])
        assert mixed[1] is None and list(mixed[0][0]) == list(four_files[0]["sizes"])
        assert list(mixed[2][0]) == list(four_files[3]["sizes"][:-1])


def test_cli_output_is_the_same_with_either_indexer(four_files, tmp_path):
    from test_gpu_decode_set import flac_file
    names = []
    for k, x in enumerate(four_files):
        flac_file(tmp_path / f"f{k}.flac", x)
        names.append(str(tmp_path / f"f{k}.flac"))
    x = four_files[2]
    flac_file(tmp_path / "cut.flac", x, x["frames"][:len(x["frames"]) - 9])           # cut inside its last frame
    names.append(str(tmp_path / "cut.flac"))
    runs = {}
    for leg, env in (("device", {}), ("host", {"FLAKE_AMD_INDEX_HOST": "1"})):
        e = {k: v for k, v in os.environ.items() if k != "FLAKE_AMD_INDEX_HOST"}
        e.update(env)
        one, many = tmp_path / f"one_{leg}", tmp_path / f"many_{leg}"
        one.mkdir(), many.mkdir()
        res = []
        for nm in names:
            base = os.path.basename(nm)[:-5]
            p = subprocess.run([CLI, "--decode", nm, str(one / f"{base}.wav")], capture_output=True, text=True, timeout=120, env=e)
            res.append((p.returncode, p.stderr, (one / f"{base}.wav").read_bytes()))
        p = subprocess.run([CLI, "--decode", "--set", str(many)] + names, capture_output=True, text=True, timeout=120, env=e)
        res.append((p.returncode, p.stderr.replace(str(many), "OUT"), [(many / f).read_bytes() for f in sorted(os.listdir(many))]))
        runs[leg] = res
    assert runs["device"] == runs["host"]
    assert [r[0] for r in runs["device"]] == [0, 0, 0, 0, 1, 1]
    for k, x in enumerate(four_files):
        assert runs["device"][k][2][44:] == x["pcm"].astype("<i2").tobytes()
    assert "cut.flac" in runs["device"][5][1] and len(runs["device"][5][2]) == 5
