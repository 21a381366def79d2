"""The host entries whose small tables travel in one block (flake_amd/csrc/table_block.h): fhip_decode_frames_segments
with md5, fhip_decode_frames_windows, fhip_decode_frames_windows_rows and fhip_index_frames, at one, two and three
segments or ranges and one and two streams.  At these counts every 4-byte table of the blocks ends on an 8-byte boundary
in one case and off it in the next, which is where a table laid over its neighbour shows.  The frames are flacgen's --
mono, 16 bits, 16 samples a block, three frames a segment -- and every answer is held to what the generator knows: the
samples, the digests, the sizes."""
import hashlib

import numpy as np
import pytest
import torch as _torch

import flake_amd
import flacgen

pytestmark = pytest.mark.gpu

V = flake_amd
N, PER_SEG, FIRST, SENT = 16, 3, 5, -1234567


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(scope="module")
def nine():
    """Nine frames numbered from FIRST: (their bytes, the samples they were written from)."""
    frames, pcm = [], []
    for k in range(3 * PER_SEG):
        x = flacgen.test_signal(N, 1, 16, seed=40 + k)
        spec = dict(kind="verbatim") if k % 2 else dict(kind="fixed", order=2, porder=1)
        frames.append(flacgen.frame(x, FIRST + k, 16, 44100, [spec]))
        pcm.append(x)
    return frames, pcm


def cut(nine, nsegs):
    """The first nsegs segments: stream, frame sizes, samples [.][1], seg_first, seg_number."""
    frames, pcm = nine[0][:PER_SEG * nsegs], nine[1][:PER_SEG * nsegs]
    s = np.frombuffer(b"".join(frames), np.uint8)
    fb = np.array([len(f) for f in frames], np.int32)
    sf = np.arange(nsegs + 1, dtype=np.int32) * PER_SEG
    num = FIRST + sf[:-1].astype(np.int64)
    return s, fb, np.concatenate(pcm), sf, num


def handle():
    return flake_amd.Encoder(flake_amd.level_params(5, channels=1, block_size=N, variable_block_size=0), max_frames=16)


@pytest.mark.parametrize("nstreams", [1, 2])
@pytest.mark.parametrize("nsegs", [1, 2, 3])
def test_segments_with_md5(nine, torch, nsegs, nstreams):
    s, fb, pcm, sf, num = cut(nine, nsegs)
    per = PER_SEG * N
    seg_stream = [k % nstreams for k in range(nsegs)]
    want = [hashlib.md5() for _ in range(nstreams)]
    for k, st in enumerate(seg_stream):
        want[st].update(pcm[k * per:(k + 1) * per].astype("<i2").tobytes())
    with handle() as enc:
        states = torch.zeros(nstreams * V.MD5_STATE_BYTES, dtype=torch.uint8, device="cuda")
        digests = torch.zeros(nstreams * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.md5_init_dev(states, nstreams)
        rc, out, ns, recs, summ, start, samples, failed, err = enc.decode_frames_segments(
            s, fb, len(pcm), sf, num, md5_states=states, md5_nstreams=nstreams, seg_stream=seg_stream)
        assert rc == V.OK, err
        assert ns == len(pcm) and np.array_equal(out, pcm) and list(summ) == [len(fb), 0, -1, 0]
        assert list(start) == [k * per for k in range(nsegs)] and list(samples) == [per] * nsegs
        assert list(failed) == [-1] * nsegs and np.all(recs["status"] == 0)
        enc.md5_final_dev(states, nstreams, digests)
        enc.sync()
        got = digests.cpu().numpy().reshape(nstreams, 16)
        assert [got[k].tobytes() for k in range(nstreams)] == [w.digest() for w in want]


SKIP, TAKE = [5, 0, 17], [20, -1, 31]           # (-1: to the segment's end)


def clips(pcm, nsegs):
    per = PER_SEG * N
    return [pcm[k * per + SKIP[k]:(k + 1) * per if TAKE[k] < 0 else k * per + SKIP[k] + TAKE[k]] for k in range(nsegs)]


@pytest.mark.parametrize("nsegs", [1, 2, 3])
def test_windows(nine, nsegs):
    s, fb, pcm, sf, num = cut(nine, nsegs)
    want = clips(pcm, nsegs)
    counts = [len(w) for w in want]
    assert counts == [20, 48, 31][:nsegs]
    with handle() as enc:
        rc, out, ns, recs, summ, start, samples, failed, err = enc.decode_frames_windows(
            s, fb, sum(counts), sf, SKIP[:nsegs], TAKE[:nsegs], seg_number=num)
        assert rc == V.OK, err
        assert ns == sum(counts) and np.array_equal(out, np.concatenate(want)) and list(summ) == [len(fb), 0, -1, 0]
        assert list(samples) == counts and list(start) == list(np.cumsum([0] + counts[:-1]))
        assert list(failed) == [-1] * nsegs


@pytest.mark.parametrize("nsegs", [1, 2, 3])
def test_windows_rows(nine, torch, nsegs):
    s, fb, pcm, sf, num = cut(nine, nsegs)
    want = clips(pcm, nsegs)
    counts = [len(w) for w in want]
    row_len = 57
    seg_row = [nsegs - 1 - k for k in range(nsegs)]           # the segments' rows in reverse, one spare row behind them
    seg_col = [3, 0, 7][:nsegs]
    rows = np.full((nsegs + 1, 1, row_len), SENT, np.int32)
    for k in range(nsegs):
        rows[seg_row[k], 0, seg_col[k]:seg_col[k] + counts[k]] = want[k][:, 0]
    with handle() as enc:
        dst = torch.full((nsegs + 1, 1, row_len), SENT, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc, _, ns, recs, summ, start, samples, failed, err = enc.decode_frames_windows_rows(
            s, fb, sum(counts), sf, SKIP[:nsegs], TAKE[:nsegs], seg_row, seg_col, dst, nsegs + 1, row_len, V.ROWS_I32,
            seg_number=num)
        assert rc == V.OK, err
        assert ns == sum(counts) and list(summ) == [len(fb), 0, -1, 0]
        assert list(samples) == counts and list(start) == list(np.cumsum([0] + counts[:-1]))
        assert list(failed) == [-1] * nsegs
        assert np.array_equal(dst.cpu().numpy(), rows)


@pytest.mark.parametrize("nranges", [1, 2, 3])
def test_index_ranges(nine, nranges):
    s, fb, pcm, sf, num = cut(nine, nranges)
    off = np.concatenate([[0], np.cumsum(fb)]).astype(np.int64)
    range_first = off[sf]
    frame_cap = len(fb) + (2 if len(fb) % 2 else 1)           # odd, with room to spare
    assert frame_cap % 2 == 1
    with handle() as enc:
        rc, sizes, r_frames, r_consumed, r_variable = enc.index_ranges(s, range_first, max_block_size=N,
                                                                       frame_cap=frame_cap, sentinel=-9)
        assert rc == V.OK
        assert list(sizes[:len(fb)]) == list(fb) and np.all(sizes[len(fb):] == -9)
        assert list(r_frames) == [PER_SEG] * nranges and list(r_variable) == [0] * nranges
        assert list(r_consumed) == list(np.diff(range_first))
