"""The packed encode fed by fhip_frames_packed_gather (flake_amd.Encoder.frames_packed_gather): the handle's PCM staging
filled through a piece table from device sources must be, to everything downstream, the batch an upload of the same
samples is -- the same frames and frame sizes from _begin, _begin_ragged and the variable-block-size entry, and K5
reading the gathered samples where they lie.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch as _torch

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
TOKEN = 0x1000                    # what names the gathered batch: compared, never followed


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def scatter(pcm, seed):
    """The samples pcm [N][ch] cut into pieces of 1 .. 100 samples, dealt to two sources with junk between them.
    Returns (the two sources as device tensors, their capacities, the piece rows)."""
    r = np.random.RandomState(seed)
    ch = pcm.shape[1]
    parts, rows, at = [[], []], [], 0
    fill = [0, 0]
    while at < len(pcm):
        n = min(int(r.choice([1, 2, 3, 5, 17, 64, 100])), len(pcm) - at)
        buf, pad = int(r.randint(0, 2)), int(r.randint(0, 4))
        parts[buf].append(r.randint(-30000, 30000, size=(pad, ch)).astype(np.int32))
        parts[buf].append(pcm[at:at + n])
        rows.append((buf, fill[buf] + pad, at, n))
        fill[buf] += pad + n
        at += n
    src = [np.ascontiguousarray(np.concatenate(p + [np.zeros((1, ch), np.int32)])) for p in parts]
    dev = [_torch.from_numpy(s).cuda() for s in src]
    _torch.cuda.synchronize()
    return dev, [len(s) for s in src], rows


def begin(enc, pcm_ptr, nframes, block_size, sizes=None, first=0):
    """fhip_frames_packed_begin(_ragged) + fetch for the batch named by pcm_ptr: (rc, bytes, frame sizes)."""
    fb = np.zeros(nframes, np.int32)
    b = V.Batch(pcm=pcm_ptr, nframes=nframes, block_size=block_size, frame_bytes=fb.ctypes.data, first_frame_number=first)
    total = C.c_int64(0)
    if sizes is None:
        rc = enc.lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total))
    else:
        sz = np.ascontiguousarray(sizes, np.int32)
        rc = enc.lib.fhip_frames_packed_begin_ragged(enc._h, C.byref(b), sz.ctypes.data, C.byref(total))
    if rc not in (V.OK, V.E_VERIFY):
        return rc, b"", fb
    out = np.zeros(max(int(total.value), 1), np.uint8)
    assert enc.lib.fhip_frames_packed_fetch(enc._h, out.ctypes.data, out.size) == V.OK
    return rc, out[:total.value].tobytes(), fb


def upload(enc, pcm, nframes, block_size, sizes=None):
    b = V.Batch(pcm=pcm.ctypes.data, nframes=nframes, block_size=block_size)
    if sizes is None:
        return enc.lib.fhip_frames_packed_upload(enc._h, C.byref(b))
    sz = np.ascontiguousarray(sizes, np.int32)
    return enc.lib.fhip_frames_packed_upload_ragged(enc._h, C.byref(b), sz.ctypes.data)


@pytest.mark.parametrize("verify", [False, True])
def test_uniform_batch_gathered_equals_uploaded(verify):
    n, nf = 64, 9
    pcm = np.ascontiguousarray(V.synth_pcm(nf, n, 2, 16, first_frame=11).reshape(-1, 2), np.int32)
    dev, caps, rows = scatter(pcm, 3)
    with V.Encoder(V.level_params(5, block_size=n), max_frames=nf) as enc:
        enc.set_verify(verify)
        assert upload(enc, pcm, nf, n) == V.OK
        rc, want, want_fb = begin(enc, pcm.ctypes.data, nf, n)
        assert rc == V.OK and len(want) == want_fb.sum() > 0
        assert enc.frames_packed_gather(TOKEN, nf, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.OK
        assert enc.last_launches() == ["k_gather_spans"]
        rc, got, got_fb = begin(enc, TOKEN, nf, n)
        assert rc == V.OK and got == want and np.array_equal(got_fb, want_fb)
        assert "k_gather_spans" not in enc.last_launches()          # _begin took the batch as it takes an upload
        # a table that does not cover exactly the batch is refused and leaves no pending batch
        assert enc.frames_packed_gather(TOKEN, nf, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows[:-1])) == V.E_INVALID
        assert enc.frames_packed_gather(TOKEN, nf + 1, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.E_INVALID
        enc.set_pcm_format(V.PCM_S16)
        assert enc.frames_packed_gather(TOKEN, nf, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.E_UNSUPPORTED


@pytest.mark.parametrize("verify", [False, True])
def test_ragged_batch_gathered_equals_uploaded(verify):
    sizes = list(range(1, 65))
    pcm = np.ascontiguousarray(V.synth_pcm(1, sum(sizes), 2, 16, first_frame=5).reshape(-1, 2), np.int32)
    dev, caps, rows = scatter(pcm, 4)
    with V.Encoder(V.level_params(5, block_size=64), max_frames=len(sizes)) as enc:
        enc.set_verify(verify)
        assert upload(enc, pcm, len(sizes), 64, sizes) == V.OK
        rc, want, want_fb = begin(enc, pcm.ctypes.data, len(sizes), 64, sizes)
        assert rc == V.OK and (want_fb > 0).all()
        assert enc.frames_packed_gather(TOKEN, len(sizes), 64, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows),
                                        block_sizes=sizes) == V.OK
        rc, got, got_fb = begin(enc, TOKEN, len(sizes), 64, sizes)
        assert rc == V.OK and got == want and np.array_equal(got_fb, want_fb)
        assert "k_gather_spans" not in enc.last_launches()
        # the uniform _begin does not take a ragged gather, and the table must add up to the sizes
        assert enc.frames_packed_gather(TOKEN, len(sizes), 64, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows),
                                        block_sizes=sizes[:-1] + [63]) == V.E_INVALID


@pytest.mark.parametrize("verify", [False, True])
def test_variable_block_size_handle(verify):
    """An allow_vbs handle: the gathered batch goes through fhip_encode_blocks_vbs_packed_numbered, block 256."""
    n, nb = 256, 5
    pcm = np.ascontiguousarray(V.synth_pcm(nb, n, 2, 16, first_frame=21).reshape(-1, 2), np.int32)
    first = np.asarray([0, 1000, 256, 77, 2 ** 31 + 5], np.uint32)
    dev, caps, rows = scatter(pcm, 6)
    with V.Encoder(V.level_params(10, block_size=n), max_frames=8 * nb) as enc:
        enc.set_verify(verify)
        want, want_bb, want_bf, want_mx = enc.encode_blocks_vbs_packed_numbered(pcm, n, first)
        assert want_bf.max() > 1                                     # some block was split
        assert enc.frames_packed_gather(TOKEN, nb, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.OK
        cap = len(want) + 4096
        out = np.zeros(cap, np.uint8)
        bb, bf, mx = (np.zeros(nb, np.int32) for _ in range(3))
        wrote = C.c_int64(0)
        rc = enc.lib.fhip_encode_blocks_vbs_packed_numbered(enc._h, TOKEN, nb, n, first.ctypes.data, out.ctypes.data, cap,
                                                            bb.ctypes.data, bf.ctypes.data, mx.ctypes.data, C.byref(wrote))
        assert rc == V.OK and out[:wrote.value].tobytes() == want.tobytes()
        assert np.array_equal(bb, want_bb) and np.array_equal(bf, want_bf) and np.array_equal(mx, want_mx)
        assert "k_gather_spans" not in enc.last_launches()


def test_k5_reads_the_gathered_pcm():
    """The frames of a gathered batch verify against the gathered samples, and with one SOURCE sample changed after the
    encode the same frames fail with SAMPLES at that very sample: the verifier read what the gather wrote."""
    n, nf = 64, 9
    pcm = np.ascontiguousarray(V.synth_pcm(nf, n, 2, 16, first_frame=31).reshape(-1, 2), np.int32)
    dev, caps, rows = scatter(pcm, 8)
    with V.Encoder(V.level_params(5, block_size=n), max_frames=nf) as enc:
        enc.set_verify(True)
        assert enc.frames_packed_gather(TOKEN, nf, n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.OK
        rc, data, fb = begin(enc, TOKEN, nf, n)
        assert rc == V.OK                                            # K5 ran inside _begin, on the staging the gather filled
        stream = _torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        sizes = _torch.from_numpy(fb.copy()).cuda()
        gathered = _torch.zeros((nf * n, 2), dtype=_torch.int32, device="cuda")
        summary = _torch.zeros(4, dtype=_torch.int64, device="cuda")
        recs = _torch.zeros((nf, 4), dtype=_torch.int32, device="cuda")
        _torch.cuda.synchronize()

        def verdict():
            assert enc.gather_spans_dev(gathered, nf * n, dev[0], caps[0], dev[1], caps[1], V.gather_pieces(rows)) == V.OK
            enc.verify_frames_dev(stream, len(data), sizes, nf, gathered, nf * n, 0, summary, recs)
            enc.sync()
            return summary.cpu().numpy(), recs.cpu().numpy()

        summ, _ = verdict()
        assert list(summ) == [nf, 0, -1, 0]
        # sample 5 * 64 + 17 of the batch, right channel: find the piece that brings it and change it at its source
        target = 5 * n + 17
        buf, src, dst, cnt = next(r for r in rows if r[2] <= target < r[2] + r[3])
        dev[buf][src + target - dst, 1] += 1
        _torch.cuda.synchronize()
        summ, rec = verdict()
        assert list(summ) == [nf, 1, 5, V.V_SAMPLES]
        assert rec[5][0] == V.V_SAMPLES and rec[5][3] == 17 and (rec[:5, 0] == 0).all() and (rec[6:, 0] == 0).all()
