"""The decoding side's CPU parts: STREAMINFO read back (flake_amd_read_streaminfo) and frame discovery in a
foreign stream (flake_amd_index_frames).  Neither touches the device."""
import numpy as np
import pytest

import flake_amd
import flacgen
import goldenlib as G


def streaminfo(channels=2, bps=16, rate=44100, max_block=4096, min_block=None, samples=0, md5=None, min_frame=0,
               max_frame=0):
    si = flake_amd.HostStreaminfo()
    si.min_block_size = max_block if min_block is None else min_block
    si.max_block_size = max_block
    si.min_frame_size, si.max_frame_size = min_frame, max_frame
    si.sample_rate, si.channels, si.bits_per_sample, si.samples = rate, channels, bps, samples
    for i, b in enumerate(md5 or bytes(16)):
        si.md5sum[i] = b
    return si


def fields(si):
    return ([getattr(si, k) for k, _ in flake_amd.HostStreaminfo._fields_[:8]], bytes(si.md5sum))


def test_abi_and_host_symbols():
    for n in ("fhip_decode_frames", "fhip_decode_frames_dev"):
        assert n in flake_amd.ABI_SYMBOLS and hasattr(flake_amd.load_library(), n)
    lib = flake_amd.load_host_library()
    for n in ("flake_amd_read_streaminfo", "flake_amd_index_frames", "flake_amd_decode_open", "flake_amd_decode_frames",
              "flake_amd_decode_md5", "flake_amd_decode_last_error", "flake_amd_decode_close"):
        assert hasattr(lib, n), n
    assert flake_amd.C.sizeof(flake_amd.DecodeIn) == 40 and flake_amd.C.sizeof(flake_amd.DecodeOut) == 40


@pytest.mark.parametrize("kw", [
    dict(),
    dict(channels=8, bps=32, rate=655350, max_block=65535, min_block=16, samples=0xFFFFFFFF, md5=bytes(range(1, 17)),
         min_frame=0xFFFFFF, max_frame=0xABCDEF),
    dict(channels=1, bps=4, rate=1, max_block=16, samples=1),
    dict(channels=2, bps=24, rate=96000, max_block=4608, samples=123456789, md5=bytes([0xFF] * 16), max_frame=14000),
])
def test_streaminfo_round_trip(kw):
    si = streaminfo(**kw)
    data = flake_amd.write_streaminfo(si)
    back, hi = flake_amd.read_streaminfo(data)
    assert hi == 0
    assert fields(back) == fields(si)
    assert flake_amd.write_streaminfo(back) == data


def test_streaminfo_36_bit_sample_count():
    """The format's sample count has 36 bits, the struct's field (libflake's layout) 32: the upper four come back as
    the return value."""
    total = (0xB << 32) | 0x89ABCDEF
    si = streaminfo(channels=2, bps=32, samples=total & 0xFFFFFFFF)
    data = bytearray(flake_amd.write_streaminfo(si))
    assert data[13] & 15 == 0
    data[13] |= total >> 32
    back, hi = flake_amd.read_streaminfo(bytes(data))
    assert (hi << 32) | back.samples == total
    assert fields(back) == fields(si)


def test_streaminfo_rejects_what_no_stream_carries():
    data = bytearray(flake_amd.write_streaminfo(streaminfo()))
    data[10] = data[11] = 0
    data[12] &= 0x0F                     # sample rate 0
    with pytest.raises(ValueError):
        flake_amd.read_streaminfo(bytes(data))
    assert flake_amd.load_host_library().flake_amd_read_streaminfo(None, None) == -1


# ---- indexing ------------------------------------------------------------------------------------

SUB = [dict(kind="fixed", order=2, porder=0)]


def fixed_stream(sizes, first=0, bps=16, nch=1, seed=0):
    """Frames of a fixed-block stream, numbered first, first + 1, ...: (frames, pcm)."""
    frames, pcm = [], []
    for i, n in enumerate(sizes):
        x = flacgen.test_signal(n, nch, bps, seed=seed + i)
        frames.append(flacgen.frame(x, first + i, bps, 44100, SUB * nch))
        pcm.append(x)
    return frames, pcm


def vbs_stream(sizes, first=0, bps=16, seed=0):
    frames, at = [], first
    for i, n in enumerate(sizes):
        x = flacgen.test_signal(n, 1, bps, seed=seed + i)
        frames.append(flacgen.frame(x, at, bps, 44100, SUB, vbs=True))
        at += n
    return frames


def check_index(si, frames, stream=None):
    stream = b"".join(frames) if stream is None else stream
    got = flake_amd.index_frames(si, stream)
    assert got is not None
    sizes, used = got
    assert list(sizes) == [len(f) for f in frames]
    assert used == sum(len(f) for f in frames)
    return sizes, used


def test_index_fixed_blocks_with_short_last_frame():
    frames, _ = fixed_stream([1152] * 5 + [200], first=7)
    check_index(streaminfo(channels=1, max_block=1152), frames)


def test_index_variable_blocks():
    frames = vbs_stream([256, 1000, 192, 17], first=(1 << 31) - 300)
    check_index(streaminfo(channels=1, max_block=4096, min_block=16), frames)


def test_index_in_pieces_and_cap():
    frames, _ = fixed_stream([192] * 7, first=0)
    si = streaminfo(channels=1, max_block=192)
    stream = b"".join(frames)
    sizes, used = flake_amd.index_frames(si, stream, cap=3)
    assert list(sizes) == [len(f) for f in frames[:3]] and used == sum(len(f) for f in frames[:3])
    rest, used2 = flake_amd.index_frames(si, stream[used:])
    assert list(rest) == [len(f) for f in frames[3:]] and used + used2 == len(stream)
    none, used0 = flake_amd.index_frames(si, b"")
    assert len(none) == 0 and used0 == 0


def test_index_skips_a_decoy_header():
    """A VERBATIM subframe whose payload is the byte image of a complete valid header -- CRC-8 included, carrying the
    expected next number: the CRC-16 of the span up to it fails, so it is no frame boundary."""
    n, bps = 192, 16
    good_next = flacgen.frame(flacgen.test_signal(n, 1, bps, seed=5), 4, bps, 44100, SUB)
    hdr = good_next[:6]                          # sync, codes, number 4, CRC-8: a whole header (block size from the table)
    assert flacgen.crc8(hdr[:5]) == hdr[5]
    x = flacgen.test_signal(n, 1, bps, seed=6)
    # verbatim samples are 16 bits each and start on a byte boundary (8 header bits of the subframe after 6 whole
    # header bytes): samples 10..12 spell the header
    for k in range(3):
        v = (hdr[2 * k] << 8) | hdr[2 * k + 1]
        x[10 + k, 0] = v - (1 << 16) if v >= 1 << 15 else v
    decoy = flacgen.frame(x, 3, bps, 44100, [dict(kind="verbatim")])
    at = decoy.find(hdr)
    assert at > 6 and decoy[at:at + 6] == hdr
    before, _ = fixed_stream([n] * 3, first=0)
    frames = before + [decoy, good_next]
    si = streaminfo(channels=1, max_block=n)
    check_index(si, frames)
    # the same header at that place IS a boundary once the span's CRC-16 holds: the search is not blind to it
    body = decoy[:at - 2]
    split = body + flacgen.crc16(body).to_bytes(2, "big")
    sizes, used = flake_amd.index_frames(si, b"".join(before) + split + decoy[at:])
    assert list(sizes[:4]) == [len(f) for f in before] + [len(split)]


def test_index_stops_before_a_cut_frame():
    frames, _ = fixed_stream([1152] * 4, first=0)
    si = streaminfo(channels=1, max_block=1152)
    stream = b"".join(frames)
    cut = stream[:len(stream) - len(frames[-1]) // 2]
    sizes, used = flake_amd.index_frames(si, cut)
    assert list(sizes) == [len(f) for f in frames[:3]]
    assert used == sum(len(f) for f in frames[:3])
    # ... and a corrupted byte in the last frame: its CRC-16 no longer holds at the end
    bad = bytearray(stream)
    bad[-20] ^= 0x10
    sizes, used = flake_amd.index_frames(si, bytes(bad))
    assert len(sizes) == 3 and used == sum(len(f) for f in frames[:3])


def test_index_garbage_first():
    frames, _ = fixed_stream([192] * 2)
    si = streaminfo(channels=1, max_block=192)
    assert flake_amd.index_frames(si, b"\x00\x01\x02" + b"".join(frames)) is None
    assert flake_amd.index_frames(si, b"\xff\xf8" + bytes(40)) is None
    # a good stream of another format is garbage to this STREAMINFO
    assert flake_amd.index_frames(streaminfo(channels=2, max_block=192), b"".join(frames)) is None


def test_index_numbers_must_continue():
    a, _ = fixed_stream([192] * 2, first=0)
    b, _ = fixed_stream([192] * 2, first=9, seed=4)
    si = streaminfo(channels=1, max_block=192)
    sizes, used = flake_amd.index_frames(si, b"".join(a + b))
    # frame 1 cannot end at the header that carries 9: no boundary is placed there.  (The CRC-16 of whole frames back
    # to back holds at their end -- each frame's own CRC returns the register to zero -- so the rest of the stream is
    # reported as one span that ends at `bytes`, which the decoder then refuses.)
    assert sizes[0] == len(a[0])
    assert len(a[0]) + len(a[1]) not in list(np.cumsum(sizes))
    cut = b"".join(a + b)[:-5]
    sizes, used = flake_amd.index_frames(si, cut)
    assert list(sizes) == [len(a[0])] and used == len(a[0])


def test_index_golden_reference_streams():
    z = G.load("ref_path.npz")
    seen = 0
    for key in z.keys():
        if not key.startswith("frames_"):
            continue
        name = key[len("frames_"):]
        lens = z["framelens_" + name]
        p = flake_amd.Params(*[int(v) for v in z["params_" + name]])
        if p.allow_vbs:
            continue                              # (the lengths there are per block, a block may be several frames)
        stream = z[key]
        assert int(lens.sum()) == len(stream)
        si = streaminfo(channels=p.channels, bps=p.bits_per_sample, rate=p.sample_rate, max_block=p.block_size)
        sizes, used = flake_amd.index_frames(si, stream)
        assert list(sizes) == [int(v) for v in lens], name
        assert used == len(stream)
        seen += 1
    assert seen >= 3
