"""K11's gather (fhip_gather_frames_dev: k_gather_offsets, k_gather_frames) against numpy: every accepted frame's bytes at
the exclusive prefix sum of the accepted lengths before it, dst_frame_bytes, and nothing else touched -- not the bytes
before dst, not the bytes behind the accepted total, not the destination of a frame that is not accepted.  Frame lengths
from 1 byte to more than a wave's round of 16-byte stores, every pair of source and destination residues modulo 16, a
source that is exactly its allocation, and frames above byte 2^32 of a large allocation.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as _torch

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
LENGTHS = (1, 2, 3, 15, 16, 17, 31, 33, 255, 16385)
GUARD = 64                        # sentinel bytes on either side of the destination (keeps dst 16-byte aligned)
SENTINEL = 0xA5
MAX_FRAMES = 8192


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def handle():
    return V.Encoder(V.level_params(5, block_size=192), max_frames=MAX_FRAMES)


def residue_table():
    """[(src offset, length)] and the source's size: every length at every (source, destination) residue pair, the
    destination residue set by a filler frame of 1 .. 15 bytes where the lengths before do not give it.  The first frame
    begins at byte 0 of the source and the last ends at its last byte."""
    frames, src_at, dst_at = [], 0, 0

    def put(n, sr):
        nonlocal src_at, dst_at
        at = (src_at + 15) // 16 * 16 + sr if frames else 0
        frames.append((at, n))
        src_at = at + n
        dst_at += n

    for n in LENGTHS:
        for dr in range(16):
            for sr in range(16):
                fill = (dr - dst_at) % 16
                if fill:
                    put(fill, (sr + 5) % 16)
                assert dst_at % 16 == dr
                put(n, sr)
    return frames, src_at


def run(enc, src_dev, src_bytes, frames, dst_cap, dst_base=0):
    """The call on a guarded destination.  Returns (rc, launches, the whole guarded buffer, dst_frame_bytes with its own
    guards)."""
    nf = len(frames)
    dst = _torch.full((2 * GUARD + dst_cap,), SENTINEL, dtype=_torch.uint8, device="cuda")
    fbytes = _torch.full((nf + 2,), -77, dtype=_torch.int32, device="cuda")
    f_src = _torch.from_numpy(np.array([f[0] for f in frames], np.int64)).cuda()
    f_len = _torch.from_numpy(np.array([f[1] for f in frames], np.int32)).cuda()
    _torch.cuda.synchronize()
    assert (dst.data_ptr() + GUARD) % 16 == 0
    rc = enc.gather_frames_dev(dst.data_ptr() + GUARD + dst_base, dst_cap - dst_base, fbytes.data_ptr() + 4, src_dev,
                               src_bytes, f_src, f_len, nf)
    launches = enc.last_launches()
    enc.sync()
    return rc, launches, dst.cpu().numpy(), fbytes.cpu().numpy()


def expect(src, src_bytes, frames, dst_cap, dst_base=0):
    """numpy's answer: the guarded buffer and dst_frame_bytes."""
    out = np.full(2 * GUARD + dst_cap, SENTINEL, np.uint8)
    fb, at = [], 0
    for s, n in frames:
        ok = n >= 1 and s >= 0 and s + n <= src_bytes and at + n <= dst_cap - dst_base
        fb.append(n if ok else 0)
        if ok:
            out[GUARD + dst_base + at:GUARD + dst_base + at + n] = src(s, n)
            at += n
    return out, np.array([-77, *fb, -77], np.int32), at


def test_every_length_at_every_pair_of_residues():
    frames, src_bytes = residue_table()
    assert len(frames) <= MAX_FRAMES
    assert {(s % 16, n) for s, n in frames} >= {(r, n) for r in range(16) for n in LENGTHS}
    assert frames[0][0] == 0 and frames[-1][0] + frames[-1][1] == src_bytes
    host = np.random.RandomState(11).randint(0, 256, size=src_bytes).astype(np.uint8)
    src = _torch.from_numpy(host.copy()).cuda()                  # the allocation is exactly src_bytes
    total = sum(n for _, n in frames)
    want, want_fb, at = expect(lambda s, n: host[s:s + n], src_bytes, frames, total)
    assert at == total
    # every (source, destination) residue pair is met by every length
    seen, d = set(), 0
    for s, n in frames:
        seen.add((s % 16, d % 16, n))
        d += n
    assert seen >= {(a, b, n) for a in range(16) for b in range(16) for n in LENGTHS}
    with handle() as enc:
        rc, launches, got, got_fb = run(enc, src, src_bytes, frames, total)
        assert rc == V.OK and launches == ["k_gather_offsets", "k_gather_frames"]
        assert np.array_equal(got_fb, want_fb)
        assert np.array_equal(got, want)
        # the same frames into a destination that begins at every residue: the head and tail lanes move with it
        for base in (1, 7, 15):
            rc, _, got, got_fb = run(enc, src, src_bytes, frames[:700], total + base, dst_base=base)
            w, wfb, _ = expect(lambda s, n: host[s:s + n], src_bytes, frames[:700], total + base, dst_base=base)
            assert rc == V.OK and np.array_equal(got_fb, wfb) and np.array_equal(got, w), base
        enc.set_profiling(True)
        assert run(enc, src, src_bytes, frames, total)[0] == V.OK
        times = enc.kernel_times()
        assert times["k_gather_offsets"][1] == 1 and times["k_gather_frames"][1] == 1
        assert times["k_gather_offsets"][0] > 0 and times["k_gather_frames"][0] > 0


def test_frames_that_are_not_accepted_copy_nothing_and_take_no_room():
    src_bytes = 5000
    host = np.random.RandomState(12).randint(0, 256, size=src_bytes).astype(np.uint8)
    src = _torch.from_numpy(host.copy()).cuda()
    frames = [(0, 100), (4990, 11), (300, 0), (-1, 10), (4990, 10), (200, -5), (1000, 3000), (40, 33), (5000, 1),
              (1 << 40, 7), (77, 17)]
    dst_cap = 100 + 10 + 33 + 17 + 50                            # the 3000-byte frame does not fit, the later ones do
    want, want_fb, at = expect(lambda s, n: host[s:s + n], src_bytes, frames, dst_cap)
    assert want_fb[1:-1].tolist() == [100, 0, 0, 0, 10, 0, 0, 33, 0, 0, 17] and at == 160
    with handle() as enc:
        rc, _, got, got_fb = run(enc, src, src_bytes, frames, dst_cap)
        assert rc == V.OK and np.array_equal(got_fb, want_fb) and np.array_equal(got, want)
        # a destination of no room at all
        rc, _, got, got_fb = run(enc, src, src_bytes, frames, 0)
        assert rc == V.OK and not got_fb[1:-1].any() and (got == SENTINEL).all()


def test_a_frame_that_does_not_fit_in_a_later_round_of_the_scan():
    """More frames than one round of k_gather_offsets' workgroup: the frame that does not fit lies in the second round,
    and the rounds behind it are placed as if it were not there."""
    r = np.random.RandomState(13)
    src_bytes = 1 << 16
    host = r.randint(0, 256, size=src_bytes).astype(np.uint8)
    src = _torch.from_numpy(host.copy()).cuda()
    frames = [(int(r.randint(0, src_bytes - 40)), int(r.randint(1, 40))) for _ in range(3500)]
    frames[1500] = (0, 60000)
    frames[1501] = (5, 0)
    dst_cap = sum(n for _, n in frames) - 60000
    want, want_fb, at = expect(lambda s, n: host[s:s + n], src_bytes, frames, dst_cap)
    assert at == dst_cap and want_fb[1501] == 0 and want_fb[1502] == 0
    with handle() as enc:
        rc, _, got, got_fb = run(enc, src, src_bytes, frames, dst_cap)
        assert rc == V.OK and np.array_equal(got_fb, want_fb) and np.array_equal(got, want)


def test_refusals_queue_nothing():
    src = _torch.zeros(64, dtype=_torch.uint8, device="cuda")
    with handle() as enc:
        ok = run(enc, src, 64, [(0, 8)], 8)
        assert ok[0] == V.OK
        dst = _torch.full((64,), SENTINEL, dtype=_torch.uint8, device="cuda")
        fb = _torch.full((4,), -77, dtype=_torch.int32, device="cuda")
        t64, t32 = _torch.zeros(4, dtype=_torch.int64, device="cuda"), _torch.ones(4, dtype=_torch.int32, device="cuda")
        for args in ((None, 64, fb, src, 64, t64, t32, 4), (dst, 64, None, src, 64, t64, t32, 4),
                     (dst, 64, fb, None, 64, t64, t32, 4), (dst, 64, fb, src, 64, None, t32, 4),
                     (dst, 64, fb, src, 64, t64, None, 4), (dst, -1, fb, src, 64, t64, t32, 4),
                     (dst, 64, fb, src, -1, t64, t32, 4), (dst, 64, fb, src, 64, t64, t32, -1),
                     (dst, 64, fb, src, 64, t64, t32, MAX_FRAMES + 1)):
            assert enc.gather_frames_dev(*args) == V.E_INVALID, args[1::2]
            assert enc.last_launches() == []
        assert enc.gather_frames_dev(dst, 64, fb, src, 64, t64, t32, 0) == V.OK and enc.last_launches() == []
        enc.sync()
        assert (dst.cpu().numpy() == SENTINEL).all() and (fb.cpu().numpy() == -77).all()


def test_frames_above_byte_2_to_the_32_of_a_large_allocation():
    """Offsets are 64-bit: frames at and above byte 2^32 of a 4.5 GiB allocation, the last one ending at its last byte.
    The allocation is not filled; only the frames are copied in."""
    lib = V.load_library()
    memcpy = lib.hipMemcpy                                       # (the HIP runtime the library is linked to)
    memcpy.argtypes, memcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    size = (9 << 30) // 2
    big = lib.fhip_device_alloc(size)
    assert big, "no 4.5 GiB of device memory"
    try:
        r = np.random.RandomState(14)
        frames = [((1 << 32) - 7, 40), ((1 << 32) + 1003, 16385), ((1 << 32) + (1 << 28) + 5, 255), (size - 300, 300),
                  (size - 16, 17), ((1 << 33), 1)]
        data = {}
        for s, n in frames:
            if s + n <= size:
                data[s] = r.randint(0, 256, size=n).astype(np.uint8)
                assert memcpy(big + s, data[s].ctypes.data, n, 1) == 0
        total = sum(n for s, n in frames if s + n <= size)
        want, want_fb, at = expect(lambda s, n: data[s], size, frames, total)
        assert at == total and want_fb[1:-1].tolist() == [40, 16385, 255, 300, 0, 0]
        with handle() as enc:
            rc, _, got, got_fb = run(enc, big, size, frames, total)
            assert rc == V.OK and np.array_equal(got_fb, want_fb) and np.array_equal(got, want)
    finally:
        lib.fhip_device_free(big)
