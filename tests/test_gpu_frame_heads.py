"""k_frame_heads (fhip_frame_heads_dev) against the frame-header parser of tests/test_flac_header_cpu.py, which is written
from the FLAC format and reads none of the C: record for record, for good frames and corrupt ones.  Streams are
flacgen's -- fixed and variable blocks; mono 8-bit, stereo 16-bit, 8 channels of 24 bits -- with frame starts on every
residue modulo 16, every bit of a handful of headers flipped one at a time, a last frame cut short inside its header,
sizes 0 and negative, and offsets before, across and past the stream's end.  The stream is exactly its allocation and
the records lie between sentinels."""
import functools

import numpy as np
import pytest
import torch as _torch

import flacgen
import flake_amd
from test_flac_header_cpu import reference

pytestmark = pytest.mark.gpu

V = flake_amd
RATE = 44100
GEOMETRIES = [(1, 8), (2, 16), (8, 24)]
GUARD = 4                         # sentinel records on either side of the output
FIXED_N = 192
VARIABLE_N = (16, 4096, 255, 256, 1000, 192, 576, 17, 4608, 300, 64, 1152, 2048, 5, 1024, 100, 512, 31)


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@functools.lru_cache(maxsize=None)
def frames_of(ch, bps, variable):
    """18 VERBATIM frames and their numbers: fixed blocks of 192 from frame 70000 on (a three-byte number), or blocks
    of many sizes numbered by sample from 2^31 - 3000 on (the number grows from six bytes to seven)."""
    sizes = VARIABLE_N if variable else (FIXED_N,) * len(VARIABLE_N)
    x = flacgen.test_signal(sum(sizes), ch, bps, seed=ch * 100 + bps)
    out, at, sample = [], 0, (1 << 31) - 3000
    for k, n in enumerate(sizes):
        number = sample + at if variable else 70000 + k
        out.append(flacgen.frame(x[at:at + n], number, bps, RATE, [dict(kind="verbatim")] * ch, vbs=variable))
        at += n
    return tuple(out)


def build(ch, bps, variable):
    """(stream bytes, [(offset, size)]): the frames with starts on every residue modulo 16, then the damaged copies."""
    frames = frames_of(ch, bps, variable)
    parts, table, at = [], [], 0

    def put(data, size=None, pad=0):
        nonlocal at
        parts.append(b"\xff" * pad + data)          # (padding that looks like the start of a sync code)
        table.append((at + pad, len(data) if size is None else size))
        at += pad + len(data)

    for k, f in enumerate(frames):
        want = k % 16
        put(f, pad=(want - at) % 16)
    assert {o % 16 for o, _ in table} == set(range(16))
    # every bit of the header of three frames, one at a time (the copies are the frame's first 32 bytes)
    for k in (0, 7, 17):
        f = frames[k]
        hlen = reference((ch, bps, RATE, 0), f, len(f))[2]
        for bit in range(8 * hlen):
            d = bytearray(f[:32])
            d[bit >> 3] ^= 0x80 >> (bit & 7)
            put(bytes(d), pad=bit % 3)
    # sizes that end inside the header, 0 and negative; ranges that leave the stream
    f = frames[3]
    for size in (0, -1, -(1 << 31), 1, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        put(f[:32], size=size)
    put(f[:6])                                        # the stream ends inside this header
    total = at
    table += [(total, 1), (total + 5, 40), (total - 4, 40), (-1, 40), (-(1 << 40), 40), (1 << 40, 40), (total - 9, 10),
              (0, total + 1), (0, (1 << 31) - 1)]
    return b"".join(parts), table


def expected(fmt, stream, table):
    out = np.zeros(len(table), dtype=V.FRAME_HEAD_DTYPE)
    for k, (off, size) in enumerate(table):
        if size <= 0 or off < 0 or off + size > len(stream):
            continue
        r = reference(fmt, stream[off:off + size], size)
        if r is not None:
            n, vbs, hlen, number = r
            out[k] = (number, n, 1 | (vbs << 1) | (hlen << 8))
    return out


def run(enc, stream, table, max_block_size):
    nf = len(table)
    dev = _torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()       # exactly the stream
    off = _torch.from_numpy(np.array([t[0] for t in table], np.int64)).cuda()
    size = _torch.from_numpy(np.array([t[1] for t in table], np.int32)).cuda()
    heads = _torch.full(((nf + 2 * GUARD) * 16,), 0x5A, dtype=_torch.uint8, device="cuda")
    _torch.cuda.synchronize()
    rc = enc.frame_heads_dev(dev, len(stream), off, size, nf, max_block_size, heads.data_ptr() + 16 * GUARD)
    launches = enc.last_launches()
    enc.sync()
    return rc, launches, heads.cpu().numpy()


@pytest.mark.parametrize("variable", [False, True], ids=["fixed", "variable"])
@pytest.mark.parametrize("ch,bps", GEOMETRIES)
def test_heads_are_what_the_format_says(ch, bps, variable):
    stream, table = build(ch, bps, variable)
    p = V.level_params(5, channels=ch, bits_per_sample=bps, block_size=4608)
    with V.Encoder(p, max_frames=8) as enc:
        for max_block in (0, 1000):
            fmt = (ch, bps, RATE, max_block)
            want = expected(fmt, stream, table)
            nframes = len(frames_of(ch, bps, variable))
            good = want["flags"][:nframes] & 1
            if max_block == 0 or not variable:
                assert good.all()                                 # the generator's frames are frames of this format
            else:
                assert good.any() and not good.all()              # the limit refuses the longer blocks
            damaged = want["flags"][nframes:] & 1
            assert damaged.any() and not damaged.all()            # (the copies cut at or behind the header's end are good)
            rc, launches, got = run(enc, stream, table, max_block)
            assert rc == V.OK and launches == ["k_frame_heads"]
            assert (got[:16 * GUARD] == 0x5A).all() and (got[-16 * GUARD:] == 0x5A).all()
            recs = got[16 * GUARD:-16 * GUARD].view(V.FRAME_HEAD_DTYPE)
            bad = np.nonzero(recs != want)[0]
            assert bad.size == 0, (bad[:5], [table[i] for i in bad[:5]], recs[bad[:5]], want[bad[:5]])


def test_another_format_s_frames_are_not_headers_of_this_one():
    stream, table = build(2, 16, False)
    with V.Encoder(V.level_params(5, channels=1, bits_per_sample=16, block_size=4608), max_frames=8) as enc:
        rc, _, got = run(enc, stream, table, 0)
        want = expected((1, 16, RATE, 0), stream, table)
        assert rc == V.OK and not (want["flags"] & 1).any()
        assert np.array_equal(got[16 * GUARD:-16 * GUARD].view(V.FRAME_HEAD_DTYPE), want)


def test_refusals_queue_nothing():
    stream, table = build(1, 8, False)
    dev = _torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).cuda()
    off = _torch.zeros(4, dtype=_torch.int64, device="cuda")
    size = _torch.ones(4, dtype=_torch.int32, device="cuda")
    heads = _torch.full((4 * 16,), 0x5A, dtype=_torch.uint8, device="cuda")
    with V.Encoder(V.level_params(5, channels=1, bits_per_sample=8, block_size=4608), max_frames=8) as enc:
        for args in ((None, 10, off, size, 4, 0, heads), (dev, 10, None, size, 4, 0, heads), (dev, 10, off, None, 4, 0, heads),
                     (dev, 10, off, size, 4, 0, None), (dev, -1, off, size, 4, 0, heads), (dev, 10, off, size, -1, 0, heads),
                     (dev, 10, off, size, 4, -1, heads)):
            assert enc.frame_heads_dev(*args) == V.E_INVALID
            assert enc.last_launches() == []
        assert enc.frame_heads_dev(dev, 10, off, size, 0, 0, heads) == V.OK and enc.last_launches() == []
        enc.sync()
        assert (heads.cpu().numpy() == 0x5A).all()
