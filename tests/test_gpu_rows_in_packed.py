"""The packed encode fed by fhip_frames_packed_from_rows (flake_amd.Encoder.frames_packed_from_rows): the handle's PCM
staging filled from a planar batch on the device must be, to everything downstream, the batch an upload of the
numpy-converted samples is -- the same frames and frame sizes from _begin and _begin_ragged, the host's MD5 from
fhip_md5_update_uploaded(_ragged), and K5 passing under fhip_set_verify.  Every comparison is exact."""
import hashlib

import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_packed_gather import begin, upload
from test_gpu_rows_in_kernel import conv

pytestmark = pytest.mark.gpu

V = flake_amd
TOKEN = 0x1000                    # what names the batch: compared, never followed
N, ROW_LEN = 256, 1027


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def rows_of(fmt, seed):
    """Three stereo rows of 16-bit audio in the format, as numpy: synthetic signal, off the grid for float32."""
    r = np.random.RandomState(seed)
    x = V.synth_pcm(3, ROW_LEN, 2, 16, first_frame=seed).reshape(3, ROW_LEN, 2).transpose(0, 2, 1)
    if fmt == V.ROWS_F32:
        return np.ascontiguousarray(x / 32768.0 + r.uniform(-0.4, 0.4, size=x.shape) / 32768.0, np.float32)
    return np.ascontiguousarray(x, np.int16 if fmt == V.ROWS_I16 else np.int32)


def laid(rows, fmt, pieces):
    """The converted samples the pieces (row, col, dst, count) lay back to back, [total][2] int32."""
    return np.ascontiguousarray(np.concatenate([conv(rows[r][:, c:c + n], fmt, 16).T for r, c, _, n in pieces]), np.int32)


def md5_uploaded(enc, nblocks, block_size=None, sizes=None):
    """One stream that absorbs every block of the pending upload in order: its digest."""
    states = _torch.zeros(V.MD5_STATE_BYTES, dtype=_torch.uint8, device="cuda")
    _torch.cuda.synchronize()
    enc.md5_init_dev(states, 1)
    first, blocks = np.array([0, nblocks], np.int32), np.arange(nblocks, dtype=np.int32)
    if sizes is None:
        rc = enc.lib.fhip_md5_update_uploaded(enc._h, states.data_ptr(), 1, nblocks, block_size, first.ctypes.data,
                                              blocks.ctypes.data)
    else:
        sz = np.ascontiguousarray(sizes, np.int32)
        rc = enc.lib.fhip_md5_update_uploaded_ragged(enc._h, states.data_ptr(), 1, nblocks, sz.ctypes.data,
                                                     first.ctypes.data, blocks.ctypes.data)
    assert rc == V.OK, enc.lib.fhip_last_error(enc._h)
    digest = np.zeros(16, np.uint8)
    assert enc.lib.fhip_md5_final(enc._h, states.data_ptr(), 1, digest.ctypes.data) == V.OK
    return digest.tobytes()


@pytest.mark.parametrize("fmt", [V.ROWS_I32, V.ROWS_I16, V.ROWS_F32])
@pytest.mark.parametrize("verify", [False, True])
def test_uniform_batch_from_rows_equals_uploaded(verify, fmt):
    """Two frames of 256 stereo samples: one from the middle of row 2, one put together from rows 0 and 1."""
    rows = rows_of(fmt, 11)
    pieces = [(2, 301, 0, N), (0, 1, N, 100), (1, ROW_LEN - 156, N + 100, 156)]
    pcm = laid(rows, fmt, pieces)
    dev = _torch.from_numpy(rows).cuda()
    _torch.cuda.synchronize()
    with V.Encoder(V.level_params(5, block_size=N), max_frames=4) as enc:
        enc.set_verify(verify)
        assert upload(enc, pcm, 2, N) == V.OK
        rc, want, want_fb = begin(enc, pcm.ctypes.data, 2, N)
        assert rc == V.OK and len(want) == want_fb.sum() > 0
        assert enc.frames_packed_from_rows(TOKEN, 2, N, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces)) == V.OK
        assert enc.last_launches() == ["k_rows_to_pcm"]
        assert md5_uploaded(enc, 2, block_size=N) == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
        rc, got, got_fb = begin(enc, TOKEN, 2, N)
        assert rc == V.OK and got == want and np.array_equal(got_fb, want_fb)
        assert "k_rows_to_pcm" not in enc.last_launches()          # _begin took the batch as it takes an upload
        # a table that does not cover exactly the batch is refused, as is what fhip_pcm_from_rows_dev refuses
        for bad in (dict(pieces=pieces[:-1]), dict(nframes=3), dict(nrows=1), dict(row_len=ROW_LEN - 1), dict(fmt=7),
                    dict(rows=None)):
            a = dict(token=TOKEN, nframes=2, block_size=N, rows=dev, nrows=3, row_len=ROW_LEN, fmt=fmt, pieces=pieces)
            a.update(bad)
            a["pieces"] = V.row_pieces(a["pieces"])
            assert enc.frames_packed_from_rows(**a) == V.E_INVALID and enc.last_launches() == [], bad
        enc.set_pcm_format(V.PCM_S16)
        assert enc.frames_packed_from_rows(TOKEN, 2, N, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces)) == V.E_UNSUPPORTED


@pytest.mark.parametrize("fmt", [V.ROWS_I16, V.ROWS_F32])
@pytest.mark.parametrize("verify", [False, True])
def test_ragged_batch_from_rows_equals_uploaded(verify, fmt):
    """Three frames of their own lengths, one per row, each from where its row's whole blocks end."""
    rows = rows_of(fmt, 12)
    sizes = [255, 1, 17]
    L = max(sizes)                                                         # a ragged batch's block_size: its longest block
    pieces = [(0, 3 * N, 0, 255), (1, 2 * N, 255, 1), (2, 4 * N - 14, 256, 17)]
    pcm = laid(rows, fmt, pieces)
    dev = _torch.from_numpy(rows).cuda()
    _torch.cuda.synchronize()
    with V.Encoder(V.level_params(5, block_size=N), max_frames=4) as enc:
        enc.set_verify(verify)
        assert upload(enc, pcm, 3, L, sizes) == V.OK
        rc, want, want_fb = begin(enc, pcm.ctypes.data, 3, L, sizes)
        assert rc == V.OK and (want_fb > 0).all()
        assert enc.frames_packed_from_rows(TOKEN, 3, L, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces), block_sizes=sizes) == V.OK
        assert enc.last_launches() == ["k_rows_to_pcm"]
        assert md5_uploaded(enc, 3, sizes=sizes) == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
        rc, got, got_fb = begin(enc, TOKEN, 3, L, sizes)
        assert rc == V.OK and got == want and np.array_equal(got_fb, want_fb)
        assert "k_rows_to_pcm" not in enc.last_launches()
        # the table must add up to the sizes
        assert enc.frames_packed_from_rows(TOKEN, 3, L, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces),
                                           block_sizes=[255, 1, 16]) == V.E_INVALID


def test_k5_reads_the_converted_pcm():
    """With verification on, a float32 batch passes inside _begin.  The same frames verify against K12's conversion of
    the same rows into a buffer of the test's, and with one ELEMENT moved by a whole step they fail with SAMPLES at that
    very sample: the frames hold what K12 wrote."""
    fmt = V.ROWS_F32
    rows = rows_of(fmt, 13)
    pieces = [(1, 5, 0, 2 * N)]
    dev = _torch.from_numpy(rows).cuda()
    _torch.cuda.synchronize()
    with V.Encoder(V.level_params(5, block_size=N), max_frames=4) as enc:
        enc.set_verify(True)
        assert enc.frames_packed_from_rows(TOKEN, 2, N, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces)) == V.OK
        rc, data, fb = begin(enc, TOKEN, 2, N)
        assert rc == V.OK                                            # K5 ran inside _begin, on the staging K12 filled
        pcm = _torch.zeros((2 * N, 2), dtype=_torch.int32, device="cuda")
        stream = _torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        sizes = _torch.from_numpy(fb.copy()).cuda()
        summary = _torch.zeros(4, dtype=_torch.int64, device="cuda")
        recs = _torch.zeros((2, 4), dtype=_torch.int32, device="cuda")
        _torch.cuda.synchronize()

        def verdict():
            assert enc.pcm_from_rows_dev(pcm, 2 * N, dev, 3, ROW_LEN, fmt, V.row_pieces(pieces)) == V.OK
            enc.verify_frames_dev(stream, len(data), sizes, 2, pcm, 2 * N, 0, summary, recs)
            enc.sync()
            return summary.cpu().numpy(), recs.cpu().numpy()

        summ, _ = verdict()
        assert list(summ) == [2, 0, -1, 0]
        v = float(rows[1, 1, 5 + N + 17])                                    # sample 17 of frame 1, right channel
        dev[1, 1, 5 + N + 17] = v - 1.0 / 32768 if v > 0 else v + 1.0 / 32768
        _torch.cuda.synchronize()
        summ, rec = verdict()
        assert list(summ) == [2, 1, 1, V.V_SAMPLES]
        assert rec[1][0] == V.V_SAMPLES and rec[1][3] == 17 and rec[0][0] == 0
