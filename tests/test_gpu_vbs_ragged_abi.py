"""The ragged variable-block-size entries of the C ABI (fhip_encode_blocks_vbs_ragged_numbered, fhip_vbs_split_ragged,
fhip_verify_frames_blocks_ragged, the ragged upload on allow_vbs handles) against the entries that already exist:
blocks of distinct lengths in ONE call must be, byte for byte and record for record, what the existing entries write
for each block alone -- fhip_encode_blocks_vbs_packed_numbered where split_frame_v1 sees the block, the packed path
under fhip_set_block_numbering(1) otherwise -- whatever the block's position or neighbours."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import flake_amd
import vbs_ragged_inputs as I

pytestmark = pytest.mark.gpu

V = flake_amd
BS = I.BS
NUMBER = V.VERIFY_STATUS.index("NUMBER")

# level, channels, bits
CASES = [(10, 2, 16), (9, 1, 16), (12, 2, 24), (11, 8, 16), (10, 3, 24)]


@pytest.fixture(scope="module", autouse=True)
def torch():
    # (torch brings a HIP runtime of its own: it comes first, as in the other modules that ask for it)
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def firsts(lengths):
    """Each block's first-sample number in its own stream: unrelated to its neighbours', one of them just below 2^31
    (the longest number field the reference's header writer defines: encode.c:696-716 shifts a 32-bit value by 36 for
    the 7-byte form)."""
    out = [1000003 * (i + 1) for i in range(len(lengths))]
    out[3] = 0x7FFFFFFF - 2 * BS
    return out


def one_block_call(enc, blk, first):
    """The existing entries for one block alone: (bytes, block_bytes, block_frames, block_max_frame)."""
    n = blk.shape[0]
    if I.splittable(n):
        data, bb, bfr, bmx = enc.encode_blocks_vbs_packed_numbered(blk, n, [first])
        return data.tobytes(), int(bb[0]), int(bfr[0]), int(bmx[0])
    pcm = np.ascontiguousarray(blk, np.int32)
    fb = np.zeros(1, np.int32)
    num = np.ascontiguousarray([first], np.uint32)
    b = V.Batch(pcm=pcm.ctypes.data, nframes=1, block_size=n, frame_bytes=fb.ctypes.data, frame_numbers=num.ctypes.data)
    total = C.c_int64(0)
    assert enc.lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total)) == V.OK
    out = np.zeros(int(total.value), np.uint8)
    assert enc.lib.fhip_frames_packed_fetch(enc._h, out.ctypes.data, out.size) == V.OK
    return out.tobytes(), int(fb[0]), 1, int(fb[0])


def per_block(data, bb):
    pos, out = 0, []
    for n in bb:
        out.append(bytes(data[pos:pos + int(n)]))
        pos += int(n)
    assert pos == len(data)
    return out


@pytest.fixture(scope="module")
def encoded(oracle):
    """Every case once: the ragged call forwards and reversed, the one-block calls, the device's split."""
    out = {}
    for level, ch, bits in CASES:
        lengths = I.lengths_for(level)
        blocks = I.make_blocks(100 + level * 10 + ch, lengths, ch, bits)
        splits = I.oracle_splits(oracle, blocks, ch)
        offs = {o % 16 for n, o in zip(lengths, I.byte_offsets(lengths, ch)) if I.splittable(n)}
        want = {1: {0, 4, 8, 12}, 2: {0, 8}}.get(ch)
        assert want is None or offs == want, (ch, offs)
        assert ch != 3 or any(o % 8 for o in offs), offs
        first = firsts(lengths)
        p = V.level_params(level, channels=ch, bits_per_sample=bits, block_size=BS)
        with V.Encoder(p, max_frames=8 * len(lengths)) as enc:
            enc.set_block_numbering(True)
            pcm = np.concatenate(blocks)
            data, bb, bfr, bmx = enc.encode_blocks_vbs_ragged_numbered(pcm, lengths, first)
            launches = enc.last_launches()
            rdata, rbb, rbfr, rbmx = enc.encode_blocks_vbs_ragged_numbered(np.concatenate(blocks[::-1]), lengths[::-1],
                                                                           first[::-1])
            nfr, sizes = enc.vbs_split_ragged(pcm, lengths)
            enc.set_verify(True)
            vdata, vbb, _, _ = enc.encode_blocks_vbs_ragged_numbered(pcm, lengths, first)
            enc.set_verify(False)
            uni = [one_block_call(enc, blocks[i], first[i]) for i in range(len(blocks))]
        out[(level, ch, bits)] = dict(p=p, lengths=lengths, blocks=blocks, splits=splits, first=first, pcm=pcm,
                                      data=data.tobytes(), bb=bb, bfr=bfr, bmx=bmx, launches=launches,
                                      rev=(rdata.tobytes(), rbb, rbfr, rbmx), nfr=nfr, sizes=sizes,
                                      verified=(vdata.tobytes(), vbb), uni=uni)
    return out


@pytest.mark.parametrize("case", CASES)
def test_ragged_call_equals_the_one_block_calls(encoded, case):
    t = encoded[case]
    got = per_block(t["data"], t["bb"])
    for i, (udata, ubb, ubfr, ubmx) in enumerate(t["uni"]):
        n = t["lengths"][i]
        assert (int(t["bb"][i]), int(t["bfr"][i]), int(t["bmx"][i])) == (ubb, ubfr, ubmx), (i, n)
        assert got[i] == udata, (i, n)
    # the same blocks in reversed order: the same bytes and records per block
    rdata, rbb, rbfr, rbmx = t["rev"]
    rgot = per_block(rdata, rbb)[::-1]
    assert rgot == got
    assert list(rbb[::-1]) == list(t["bb"]) and list(rbfr[::-1]) == list(t["bfr"]) and list(rbmx[::-1]) == list(t["bmx"])
    # with verification on: OK on good input, and the same bytes
    assert t["verified"][0] == t["data"] and list(t["verified"][1]) == list(t["bb"])


@pytest.mark.parametrize("case", CASES)
def test_split_ragged_equals_the_oracle_per_block(encoded, case):
    t = encoded[case]
    for i, (nf, sizes) in enumerate(t["splits"]):
        assert int(t["nfr"][i]) == nf, (i, t["lengths"][i])
        assert list(t["sizes"][i][:nf]) == sizes and not t["sizes"][i][nf:].any(), (i, t["lengths"][i])
        assert int(t["bfr"][i]) == nf, (i, t["lengths"][i])       # the encode entry cut where the diagnostic twin says


@pytest.mark.parametrize("case", CASES)
def test_launch_list_is_the_ragged_generic_kernels(encoded, case):
    names = encoded[case]["launches"]
    assert sum(1 for n in names if n.startswith("k_vbs_split")) == 1 and "k_vbs_split ragged" in names, names
    assert "k_vbs_plan ragged" in names
    for stem in ("k_prepare", "k_autocorr", "k_encode", "k_assemble"):
        hits = [n for n in names if n.startswith(stem)]
        assert hits and all("ragged" in n for n in hits), (stem, names)
    assert not any("bins" in n for n in names), names


def crc16_table():
    tab = []
    for x in range(256):
        c = x << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005 if c & 0x8000 else c << 1) & 0xFFFF
        tab.append(c)
    return tab


CRC16 = crc16_table()


def frame_sizes(decoder, t):
    """The byte size of every frame of the stream and the index of each block's first frame.  The test decoder restores
    the input from the stream (it reports block sizes, not bytes); the frame boundaries are read off the stream itself:
    a frame ends where its CRC-16 closes (the running CRC over a whole frame is 0) in front of the next sync code, and
    there are as many frames as the entry's block_frames say."""
    ch, bits = t["p"].channels, t["p"].bits_per_sample
    pcm, nsm = decoder.decode(np.frombuffer(t["data"], np.uint8), ch, bits, t["pcm"].shape[0])
    assert (pcm == t["pcm"]).all()
    data = t["data"]
    fb, cur, crc = [], 0, 0
    for i in range(len(data)):
        crc = ((crc << 8) & 0xFFFF) ^ CRC16[(crc >> 8) ^ data[i]]
        at_end = i + 1 == len(data) or data[i + 1:i + 3] == b"\xff\xf9"
        if crc == 0 and at_end and i + 1 - cur >= 8:
            fb.append(i + 1 - cur)
            cur, crc = i + 1, 0
    assert cur == len(data)
    first_frame = np.concatenate([[0], np.cumsum(t["bfr"])])
    assert len(fb) == first_frame[-1] == len(nsm)
    return np.ascontiguousarray(fb, np.int32), first_frame


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]])
def test_verifier_block_table_with_a_length_per_block(encoded, case, decoder):
    t = encoded[case]
    fb, first_frame = frame_sizes(decoder, t)
    lengths, first = t["lengths"], t["first"]
    nfr = len(fb)
    with V.Encoder(t["p"], max_frames=8 * len(lengths)) as enc:
        ok, recs, summ, _ = enc.verify_frames_blocks_ragged(t["data"], fb, t["pcm"], first, lengths)
        assert ok and list(summ) == [nfr, 0, -1, 0] and not recs["status"].any()
        # block_first[b] off by one: NUMBER at bit 32, at the first frame of block b
        for b in (0, 5, len(lengths) - 1):
            bad = list(first); bad[b] = (bad[b] + 1) & 0xFFFFFFFF
            ok, recs, summ, _ = enc.verify_frames_blocks_ragged(t["data"], fb, t["pcm"], bad, lengths)
            f = int(first_frame[b])
            assert not ok and summ[2] == f and (int(recs["status"][f]), int(recs["bit"][f])) == (NUMBER, 32), b
            failure = enc.last_verify_failure()
            assert failure is not None and failure[2] == bad[b]
        # two neighbouring table lengths exchanged: a frame no longer ends inside its block
        swapped = list(lengths); swapped[4], swapped[5] = swapped[5], swapped[4]
        ok, recs, summ, _ = enc.verify_frames_blocks_ragged(t["data"], fb, t["pcm"], first, swapped)
        f = int(summ[2])
        assert not ok and first_frame[4] <= f < first_frame[6]
        assert (int(recs["status"][f]), int(recs["bit"][f])) == (NUMBER, 16)
        # in->nsamples short by one block: the last frame does not end at the batch's end
        short = t["pcm"][:-lengths[-1]]
        ok, recs, summ, _ = enc.verify_frames_blocks_ragged(t["data"], fb, short, first, lengths)
        assert not ok and (int(recs["status"][nfr - 1]), int(recs["bit"][nfr - 1])) == (NUMBER, 16)
        # one flipped stream byte in a chosen block: what the uniform block-table mode says of that block's frames alone
        starts = np.concatenate([[0], np.cumsum(fb)])
        for b in (1, 2, 7):
            f0, f1 = int(first_frame[b]), int(first_frame[b + 1])
            f = f0 + (f1 - f0) // 2
            at = int(starts[f]) + int(fb[f]) // 2
            bad = bytearray(t["data"]); bad[at] ^= 0x10
            ok, recs, summ, _ = enc.verify_frames_blocks_ragged(bytes(bad), fb, t["pcm"], first, lengths)
            lo, hi = int(starts[f0]), int(starts[f1])
            s0 = sum(lengths[:b])
            uok, urecs, usumm, _ = enc.verify_frames_blocks(bytes(bad[lo:hi]), fb[f0:f1], t["pcm"][s0:s0 + lengths[b]],
                                                            [first[b]], lengths[b])
            assert not ok and not uok and summ[2] == f0 + usumm[2] and summ[3] == usumm[3], b
            assert recs[f0:f1].tobytes() == urecs.tobytes(), b
            assert not recs["status"][:f0].any() and not recs["status"][f1:].any(), b


def test_verifier_on_device_tables(encoded, decoder, torch):
    t = encoded[CASES[0]]
    fb, _ = frame_sizes(decoder, t)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    start = np.concatenate([[0], np.cumsum(t["lengths"])]).astype(np.int64)
    ds, dfb, dp = dev(np.frombuffer(t["data"], np.uint8).copy()), dev(fb), dev(t["pcm"])
    dbf, dst = dev(np.asarray(t["first"], np.uint32).view(np.int32)), dev(start)
    summ = torch.zeros(4, dtype=torch.int64, device="cuda")
    with V.Encoder(t["p"], max_frames=8 * len(t["lengths"])) as enc:
        vi = V.VerifyIn(ds.data_ptr(), len(t["data"]), dfb.data_ptr(), len(fb), dp.data_ptr(), t["pcm"].shape[0], 0)
        vo = V.VerifyOut(None, summ.data_ptr())
        assert enc.lib.fhip_verify_frames_blocks_ragged_dev(enc._h, C.byref(vi), dbf.data_ptr(), len(t["lengths"]),
                                                            dst.data_ptr(), C.byref(vo)) == V.OK
        enc.sync()
        assert summ.cpu().tolist() == [len(fb), 0, -1, 0]
        # a table whose second block starts one sample late: block 0's last frame still fits, block 1's first is misnumbered
        late = start.copy(); late[1] += 1
        dst2 = dev(late)
        assert enc.lib.fhip_verify_frames_blocks_ragged_dev(enc._h, C.byref(vi), dbf.data_ptr(), len(t["lengths"]),
                                                            dst2.data_ptr(), C.byref(vo)) == V.OK
        enc.sync()
        got = summ.cpu().tolist()
        assert got[1] >= 1 and got[2] == int(t["bfr"][0]) and got[3] == NUMBER


def test_refusals_launch_nothing_and_leave_the_handle_usable(encoded):
    t = encoded[CASES[0]]
    lengths, first, pcm = t["lengths"], t["first"], t["pcm"]
    nb = len(lengths)

    def call(enc, sizes, nblocks=None, nulls=(), out_cap=None):
        nblocks = len(sizes) if nblocks is None else nblocks
        sz = np.ascontiguousarray(sizes, np.int32)
        bf = np.ascontiguousarray(first[:len(sizes)] + [0] * max(0, len(sizes) - nb), np.uint32)
        out = np.full(64 + pcm.size * 5, 0xA5, np.uint8)
        rec = [np.full(max(len(sizes), 1), -7, np.int32) for _ in range(3)]
        wrote = C.c_int64(-7)
        args = dict(pcm=pcm.ctypes.data, sizes=sz.ctypes.data, first=bf.ctypes.data, out=out.ctypes.data,
                    bb=rec[0].ctypes.data, wrote=C.byref(wrote))
        for k in nulls:
            args[k] = None
        rc = enc.lib.fhip_encode_blocks_vbs_ragged_numbered(
            enc._h, args["pcm"], nblocks, args["sizes"], args["first"], args["out"],
            out.size if out_cap is None else out_cap, args["bb"], rec[1].ctypes.data, rec[2].ctypes.data, args["wrote"])
        untouched = (out == 0xA5).all() and all((r == -7).all() for r in rec) and wrote.value in (-7, 0)
        return rc, untouched

    with V.Encoder(t["p"], max_frames=8 * nb) as enc:
        enc.set_block_numbering(True)
        good, _, _, _ = enc.encode_blocks_vbs_ragged_numbered(pcm, lengths, first)
        before = enc.last_launches()
        zero = list(lengths); zero[2] = 0
        over = list(lengths); over[2] = BS + 1
        rows = [(call(enc, zero), V.E_INVALID), (call(enc, over), V.E_INVALID),
                (call(enc, lengths + [8] * 1, nblocks=nb + 1), V.E_INVALID)]          # 8 * nblocks > max_frames
        rows += [(call(enc, lengths, nulls=(k,)), V.E_INVALID) for k in ("pcm", "sizes", "first", "out", "bb", "wrote")]
        for (rc, untouched), want in rows:
            assert rc == want and untouched
            assert enc.last_launches() == before                 # nothing was queued: no new list was started
        # int32 only, as every variable-block-size entry
        enc.set_pcm_format(V.PCM_S16)
        rc, untouched = call(enc, lengths)
        assert rc == V.E_UNSUPPORTED and untouched and enc.last_launches() == before
        enc.set_pcm_format(V.PCM_S32)
        # an out_cap that is too small: as fhip_encode_blocks_vbs_packed_numbered, E_INVALID and nothing written
        rc, _ = call(enc, lengths, out_cap=16)
        assert rc == V.E_INVALID
        again, _, _, _ = enc.encode_blocks_vbs_ragged_numbered(pcm, lengths, first)
        assert again.tobytes() == good.tobytes() == t["data"]
        # the ragged packed entries stay refused on such a handle
        fbb = np.zeros(2, np.int32)
        b = V.Batch(pcm=pcm.ctypes.data, nframes=2, block_size=max(lengths[:2]), frame_bytes=fbb.ctypes.data)
        sz = np.ascontiguousarray(lengths[:2], np.int32)
        total = C.c_int64(0)
        assert enc.lib.fhip_frames_packed_begin_ragged(enc._h, C.byref(b), sz.ctypes.data, C.byref(total)) == V.E_UNSUPPORTED
        num = np.zeros(2, np.uint32); summary = np.zeros(4, np.int64); st = np.zeros(16, np.uint8)
        vi = V.VerifyIn(st.ctypes.data, 16, fbb.ctypes.data, 2, pcm.ctypes.data, sum(lengths[:2]), 0)
        vo = V.VerifyOut(None, summary.ctypes.data)
        assert enc.lib.fhip_verify_frames_ragged(enc._h, C.byref(vi), num.ctypes.data, sz.ctypes.data, C.byref(vo)) == V.E_UNSUPPORTED
    # a handle without variable block size
    with V.Encoder(V.level_params(5, block_size=BS), max_frames=8 * nb) as enc:
        rc, untouched = call(enc, lengths)
        assert rc == V.E_INVALID and untouched and enc.last_launches() == []
    # above the ragged K3's limit: callers fall back to one call per length
    with V.Encoder(V.level_params(10, block_size=20000), max_frames=16) as enc:
        rc, untouched = call(enc, lengths[:2])
        assert rc == V.E_UNSUPPORTED and untouched and enc.last_launches() == []


def test_md5_of_a_ragged_upload_then_the_encode_consumes_it(encoded, torch):
    t = encoded[CASES[0]]
    lengths, first, pcm, blocks = t["lengths"], t["first"], t["pcm"], t["blocks"]
    nb, nstreams = len(lengths), 4
    owner = [i % nstreams for i in range(nb)]
    rows = [[i for i, o in enumerate(owner) if o == s] for s in range(nstreams)]
    seg_first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.int32)
    seg = np.ascontiguousarray([i for r in rows for i in r], np.int32)
    msgs = [b"".join(np.ascontiguousarray(blocks[i].astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :2].tobytes()
                     for i in r) for r in rows]
    sz = np.ascontiguousarray(lengths, np.int32)
    pcm = np.ascontiguousarray(pcm, np.int32).copy()              # (written below)
    with V.Encoder(t["p"], max_frames=8 * nb) as enc:
        states = torch.zeros(nstreams * V.MD5_STATE_BYTES, dtype=torch.uint8, device="cuda")
        enc.md5_init_dev(states, nstreams)
        enc.sync()
        b = V.Batch(pcm=pcm.ctypes.data, nframes=nb, block_size=max(lengths))
        assert enc.lib.fhip_frames_packed_upload_ragged(enc._h, C.byref(b), sz.ctypes.data) == V.OK
        assert enc.lib.fhip_md5_update_uploaded_ragged(enc._h, states.data_ptr(), nstreams, nb, sz.ctypes.data,
                                                       seg_first.ctypes.data, seg.ctypes.data) == V.OK
        assert any("ragged general" in n for n in enc.last_launches())
        # the encode entry takes the upload over -- no second copy of the PCM: the host buffer is cleared in place
        # first, and the frames are still those of the samples that were uploaded
        pcm[:] = 0
        data, bb, _, _ = enc.encode_blocks_vbs_ragged_numbered(pcm, lengths, first)
        assert data.tobytes() == t["data"]
        assert not any("md5" in n for n in enc.last_launches())
        # the upload is consumed: an MD5 update finds none
        assert enc.lib.fhip_md5_update_uploaded_ragged(enc._h, states.data_ptr(), nstreams, nb, sz.ctypes.data,
                                                       seg_first.ctypes.data, seg.ctypes.data) == V.E_INVALID
        digests = np.zeros((nstreams, 16), np.uint8)
        assert enc.lib.fhip_md5_final(enc._h, states.data_ptr(), nstreams, digests.ctypes.data) == V.OK
        for s in range(nstreams):
            assert digests[s].tobytes() == hashlib.md5(msgs[s]).digest(), s
