"""The ragged entries of the C ABI (fhip_frames_packed_*_ragged, fhip_verify_frames_ragged,
fhip_md5_update_uploaded_ragged) against the uniform entries that already exist: N frames of distinct lengths in one
ragged call must be, byte for byte and record for record, what N uniform one-frame calls produce."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd

BS = 1152
LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, 8, 9, 77, 102, 255, 256, 257, 576, 1000, BS - 1, BS]


def blocks(ch, bits, lengths, seed=0):
    return [np.ascontiguousarray(V.synth_pcm(1, BS, ch, bits, first_frame=seed + 7 * i).reshape(-1, ch)[:n])
            for i, n in enumerate(lengths)]


def packed_call(enc, fn_name, pcm, nframes, block_size, numbers, sizes=None):
    """fhip_frames_packed_begin(_ragged) + fetch on host arrays: (rc, bytes, frame_bytes, info)."""
    ch = enc.params.channels
    pcm = np.ascontiguousarray(pcm, dtype=enc.pcm_dtype)
    fb = np.zeros(nframes, np.int32)
    info = np.zeros(nframes * ch, V.INFO_DTYPE)
    num = np.ascontiguousarray(numbers, np.uint32)
    b = V.Batch(pcm=pcm.ctypes.data, nframes=nframes, block_size=block_size, info=info.ctypes.data,
                frame_bytes=fb.ctypes.data, frame_numbers=num.ctypes.data)
    total = C.c_int64(0)
    if sizes is None:
        rc = enc.lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total))
    else:
        sz = np.ascontiguousarray(sizes, np.int32)
        rc = getattr(enc.lib, fn_name)(enc._h, C.byref(b), sz.ctypes.data, C.byref(total))
    if rc not in (V.OK, V.E_VERIFY):
        return rc, b"", fb, info
    out = np.zeros(max(int(total.value), 1), np.uint8)
    assert enc.lib.fhip_frames_packed_fetch(enc._h, out.ctypes.data, out.size) == V.OK
    return rc, out[:total.value].tobytes(), fb, info


CASES = [(2, 16, 5, V.PCM_S16), (2, 16, 8, V.PCM_S32), (1, 16, 5, V.PCM_S16), (3, 24, 2, V.PCM_S32),
         (3, 16, 0, V.PCM_S16), (2, 24, 5, V.PCM_S32)]


@pytest.fixture(scope="module")
def encoded():
    """Every case once: the ragged call, the uniform one-frame calls, the inputs."""
    out = {}
    for ch, bits, level, fmt in CASES:
        p = V.level_params(level, channels=ch, bits_per_sample=bits, block_size=BS)
        blk = blocks(ch, bits, LENGTHS)
        numbers = [3 + 5 * i for i in range(len(LENGTHS))]
        with V.Encoder(p, max_frames=len(LENGTHS)) as enc:
            enc.set_pcm_format(fmt)
            rc, data, fb, info = packed_call(enc, "fhip_frames_packed_begin_ragged", np.concatenate(blk), len(blk),
                                             max(LENGTHS), numbers, LENGTHS)
            launches = enc.last_launches()
            uni = [packed_call(enc, None, blk[i], 1, LENGTHS[i], [numbers[i]]) for i in range(len(blk))]
        out[(ch, bits, level, fmt)] = (p, blk, numbers, rc, data, fb, info, launches, uni)
    return out


@pytest.mark.parametrize("case", CASES)
def test_ragged_begin_equals_uniform_one_frame_calls(encoded, case):
    p, blk, numbers, rc, data, fb, info, launches, uni = encoded[case]
    ch = p.channels
    assert rc == V.OK
    assert all("ragged" in name for name in launches if name.startswith(("k_prepare", "k_autocorr", "k_encode", "k_assemble")))
    assert any(name.startswith("k_encode<") and "ragged" in name for name in launches), launches
    pos = 0
    for i, (urc, udata, ufb, uinfo) in enumerate(uni):
        assert urc == V.OK
        assert fb[i] == ufb[0] == len(udata), (i, LENGTHS[i])
        assert data[pos:pos + fb[i]] == udata, (i, LENGTHS[i])
        assert info[i * ch:(i + 1) * ch].tobytes() == uinfo.tobytes(), (i, LENGTHS[i])
        pos += int(fb[i])
    assert pos == len(data)


def verify_ragged(enc, stream, fb, pcm, numbers, sizes):
    ok, recs, summary, _ = enc.verify_frames_ragged(stream, fb, pcm, numbers, sizes)
    return (V.OK if ok else V.E_VERIFY), recs, summary


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_ragged_verify_accepts_and_reports_as_the_numbered_verifier(encoded, case):
    p, blk, numbers, _, data, fb, _, _, uni = encoded[case]
    fmt = case[3]
    pcm = np.concatenate(blk)
    with V.Encoder(p, max_frames=len(LENGTHS)) as enc:
        enc.set_pcm_format(fmt)
        rc, recs, summary = verify_ragged(enc, data, fb, pcm, numbers, LENGTHS)
        assert rc == V.OK and list(summary) == [len(LENGTHS), 0, -1, 0]
        assert (recs["status"] == 0).all()
        starts = np.concatenate([[0], np.cumsum(fb)])
        for i in (5, 10, 13, len(LENGTHS) - 2):
            n = LENGTHS[i]
            udata = uni[i][1]

            def uniform(stream, ufb, upcm):
                # the same corruption of the uniform one-frame call, on a handle whose block size is the frame's
                pu = V.level_params(case[2], channels=p.channels, bits_per_sample=p.bits_per_sample, block_size=n)
                with V.Encoder(pu, max_frames=1) as eu:
                    eu.set_pcm_format(fmt)
                    ok, r, s, _ = eu.verify_frames(stream, ufb, upcm, frame_numbers=[numbers[i]])
                    return int(r["status"][0]), int(r["bit"][0])

            # the size entry of one frame is changed
            fb2 = fb.copy(); fb2[i] -= 1
            rc, recs, summary = verify_ragged(enc, data, fb2, pcm, numbers, LENGTHS)
            want = uniform(udata, [len(udata) - 1], blk[i])
            assert rc == V.E_VERIFY and summary[2] == i
            assert (int(recs["status"][i]), int(recs["bit"][i])) == want, (i, n)
            # the PCM is shifted by one sample
            shifted = np.concatenate([pcm[1:], pcm[:1]])
            rc, recs, summary = verify_ragged(enc, data, fb, shifted, numbers, LENGTHS)
            assert rc == V.E_VERIFY
            sh_block = shifted[sum(LENGTHS[:i]):sum(LENGTHS[:i + 1])]
            want = uniform(udata, [len(udata)], sh_block)
            assert (int(recs["status"][i]), int(recs["bit"][i])) == want, (i, n)
            # one stream byte is flipped
            bad = bytearray(data); at = int(starts[i]) + int(fb[i]) // 2; bad[at] ^= 0x10
            ubad = bytearray(udata); ubad[int(fb[i]) // 2] ^= 0x10
            rc, recs, summary = verify_ragged(enc, bytes(bad), fb, pcm, numbers, LENGTHS)
            want = uniform(bytes(ubad), [len(udata)], blk[i])
            assert rc == V.E_VERIFY and summary[1] == 1 and summary[2] == i
            assert (int(recs["status"][i]), int(recs["bit"][i])) == want, (i, n)
        # a frame that holds another length than its table entry
        sizes2 = list(LENGTHS); sizes2[4], sizes2[5] = sizes2[4] + 1, sizes2[5] - 1
        rc, recs, summary = verify_ragged(enc, data, fb, pcm, numbers, sizes2)
        assert rc == V.E_VERIFY and int(recs["status"][4]) == V.VERIFY_STATUS.index("NUMBER") and int(recs["bit"][4]) == 16
        # a frame that carries another number
        num2 = list(numbers); num2[7] += 1
        rc, recs, summary = verify_ragged(enc, data, fb, pcm, num2, LENGTHS)
        assert rc == V.E_VERIFY and summary[2] == 7 and int(recs["status"][7]) == V.VERIFY_STATUS.index("NUMBER") and int(recs["bit"][7]) == 32


@pytest.mark.parametrize("ch,bits,fmt", [(2, 16, V.PCM_S16), (1, 16, V.PCM_S16), (3, 24, V.PCM_S32), (2, 16, V.PCM_S32)])
def test_md5_of_a_ragged_upload_equals_hashlib(ch, bits, fmt):
    import torch
    p = V.level_params(5, channels=ch, bits_per_sample=bits, block_size=BS)
    blk = blocks(ch, bits, LENGTHS, seed=11)
    nstreams = 5
    owner = [i % nstreams for i in range(len(blk))]
    owner[3] = 0                                                 # stream 3 % 5 gets one block less, stream 0 one more
    nb = (bits + 7) // 8
    with V.Encoder(p, max_frames=len(blk)) as enc:
        enc.set_pcm_format(fmt)
        states = torch.zeros(nstreams * V.MD5_STATE_BYTES, dtype=torch.uint8, device="cuda")
        enc.md5_init_dev(states, nstreams)
        enc.sync()
        pcm = np.ascontiguousarray(np.concatenate(blk), dtype=enc.pcm_dtype)
        sz = np.ascontiguousarray(LENGTHS, np.int32)
        b = V.Batch(pcm=pcm.ctypes.data, nframes=len(blk), block_size=max(LENGTHS))
        rows = [[i for i, o in enumerate(owner) if o == s] for s in range(nstreams)]
        first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.int32)
        seg = np.ascontiguousarray([i for r in rows for i in r], np.int32)
        msgs = [b"".join(np.ascontiguousarray(blk[i].astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()
                         for i in r) for r in rows]
        for rep in range(2):                                     # twice: the second update starts from partial blocks
            assert enc.lib.fhip_frames_packed_upload_ragged(enc._h, C.byref(b), sz.ctypes.data) == V.OK
            # a table that is not the upload's is refused
            sz_bad = sz.copy(); sz_bad[2] += 1
            assert enc.lib.fhip_md5_update_uploaded_ragged(enc._h, states.data_ptr(), nstreams, len(blk), sz_bad.ctypes.data,
                                                           first.ctypes.data, seg.ctypes.data) == V.E_INVALID
            assert enc.lib.fhip_md5_update_uploaded_ragged(enc._h, states.data_ptr(), nstreams, len(blk), sz.ctypes.data,
                                                           first.ctypes.data, seg.ctypes.data) == V.OK
            assert any("ragged general" in n for n in enc.last_launches())
            digests = np.zeros((nstreams, 16), np.uint8)
            assert enc.lib.fhip_md5_final(enc._h, states.data_ptr(), nstreams, digests.ctypes.data) == V.OK
            for s in range(nstreams):
                assert digests[s].tobytes() == hashlib.md5(msgs[s] * (rep + 1)).digest(), (s, rep)


def test_table_and_handle_refusals():
    p = V.level_params(5, block_size=BS)
    blk = blocks(2, 16, [100, 200])
    pcm = np.concatenate(blk)
    with V.Encoder(p, max_frames=4) as enc:
        ok = packed_call(enc, "fhip_frames_packed_begin_ragged", pcm, 2, 200, [0, 0], [100, 200])
        assert ok[0] == V.OK
        before = enc.last_launches()
        for sizes, bsz in (([0, 200], 200), ([100, BS + 1], BS), ([100, 200], 100), ([100, 200], BS), ([-5, 200], 200)):
            rc = packed_call(enc, "fhip_frames_packed_begin_ragged", pcm, 2, bsz, [0, 0], sizes)[0]
            assert rc == V.E_INVALID, (sizes, bsz)
            assert enc.last_launches() == before                 # nothing was queued: no new list was started
            b = V.Batch(pcm=pcm.ctypes.data, nframes=2, block_size=bsz)
            sz = np.ascontiguousarray(sizes, np.int32)
            assert enc.lib.fhip_frames_packed_upload_ragged(enc._h, C.byref(b), sz.ctypes.data) == V.E_INVALID
        # the handle is still good
        again = packed_call(enc, "fhip_frames_packed_begin_ragged", pcm, 2, 200, [0, 0], [100, 200])
        assert again[0] == V.OK and again[1] == ok[1]
    pv = V.level_params(10)
    with V.Encoder(pv, max_frames=8) as enc:
        n = pv.block_size
        pcm = V.synth_pcm(1, n, 2, 16).reshape(-1, 2)
        rc = packed_call(enc, "fhip_frames_packed_begin_ragged", pcm, 2, n // 2, [0, 1], [n // 2, n // 2])[0]
        assert rc == V.E_UNSUPPORTED
        fb = np.ones(1, np.int32); num = np.zeros(1, np.uint32); summary = np.zeros(4, np.int64)
        st = np.zeros(16, np.uint8)
        vi = V.VerifyIn(st.ctypes.data, 16, fb.ctypes.data, 1, pcm.ctypes.data, n, 0)
        vo = V.VerifyOut(None, summary.ctypes.data)
        sz = np.ascontiguousarray([n], np.int32)
        assert enc.lib.fhip_verify_frames_ragged(enc._h, C.byref(vi), num.ctypes.data, sz.ctypes.data, C.byref(vo)) == V.E_UNSUPPORTED
    pbig = V.level_params(5, block_size=20000)
    with V.Encoder(pbig, max_frames=2) as enc:
        rc = packed_call(enc, "fhip_frames_packed_begin_ragged", pcm[:300], 2, 200, [0, 0], [100, 200])[0]
        assert rc == V.E_UNSUPPORTED                             # callers fall back to one call per length

