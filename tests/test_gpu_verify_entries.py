"""The verifier's host entries share one staging body (api.hip, verify_host): all four of K5's modes through ONE handle,
back to back, so that what one mode leaves in the handle's table buffer would show in the next.

Every step runs twice: on the encoder's own output (passes, summary [n, 0, -1, 0]) and with one table entry off by one
(fails at that frame with NUMBER; the text and fhip_last_verify_number name the number).  The sequence mode has no
table: its second run moves first_sample by one frame, fails at frame 0 with NUMBER, and has no number to name.  Each
host entry's summary and records equal its _dev twin's on the same data.  Empty calls return OK with [0, 0, -1, 0] and
leave the handle's launch list as the code before the shared body left it (recorded on an MI355X: the verify entries
start no list of their own, so it is the list of the encode call before them -- none on a fresh handle)."""
import ctypes as C

import numpy as np
import pytest

import flake_amd
from test_gpu_ragged_abi import blocks, packed_call
from test_gpu_set_vbs import twelve_blocks

pytestmark = pytest.mark.gpu

V = flake_amd
BS = 256
RAGGED_LENGTHS = [1, 77, BS - 1, BS, 33, 2, 100]                # odd count: the table's even-rounding matters
NUMBER = V.VERIFY_STATUS.index("NUMBER")
# what the parent commit's handles report after these calls (fhip_last_launches), recorded on an MI355X
FRESH_HANDLE_LAUNCHES = []
BEHIND_AN_ENCODE = {        # test_empty_calls' encode call on each handle, then the empty calls: the encode's list stays
    "fixed": ["k_prepare_stereo<1,1,true>", "k_autocorr_wt<2,false,0> split=2", "k_lpc_reg<8>", "k_encode_pow2<4,64,0>"],
    "vbs": ["k_vbs_split", "k_vbs_plan<block_first>", "k_prepare_stereo_bins<4> narrow",
            "k_autocorr_wt<4,false,12> split=1 tail narrow", "k_order_search<4,256,4,false>", "k_encode_pow2<4,256,3>",
            "k_order_search<12,128,4,false>", "k_encode_pow2<6,256,3>", "k_order_search<4,128,4,false>",
            "k_encode_pow2<2,256,3>", "k_order_search_bins<256,4,0> narrow", "k_encode_bins<3> narrow",
            "k_order_search<28,128,4,false>", "k_encode_pow2<14,256,3>", "k_order_search<20,128,4,false>",
            "k_encode_pow2<10,256,3>", "k_assemble bins", "k_assemble bins", "k_assemble bins", "k_frame_offsets_perm",
            "k_pack_frames_perm", "k_vbs_block_bytes"],
}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


@pytest.fixture(scope="module")
def fixed(torch):
    """The fixed-block handle's inputs: a ragged batch, a numbered batch and a sequence, encoded once."""
    p = V.level_params(5, block_size=BS)
    blk = blocks(2, 16, RAGGED_LENGTHS)
    rnum = [3 + 5 * i for i in range(len(blk))]
    pcm = V.synth_pcm(5, BS, 2, 16).reshape(-1, 2)
    nnum = [7, 2, 9, 4, 11]
    with V.Encoder(p, max_frames=16) as enc:
        rc, rdata, rfb, _ = packed_call(enc, "fhip_frames_packed_begin_ragged", np.concatenate(blk), len(blk),
                                        max(RAGGED_LENGTHS), rnum, RAGGED_LENGTHS)
        assert rc == V.OK
        rc, ndata, nfb, _ = packed_call(enc, None, pcm, 5, BS, nnum)
        assert rc == V.OK
        rc, sdata, sfb, _ = packed_call(enc, None, pcm, 5, BS, [4, 5, 6, 7, 8])
        assert rc == V.OK
    return dict(p=p, ragged=(rdata, rfb, np.concatenate(blk), rnum), numbered=(ndata, nfb, pcm, nnum),
                sequence=(sdata, sfb, pcm, 4 * BS))


@pytest.fixture(scope="module")
def vbs(oracle, torch):
    """The allow_vbs handle's inputs: the first blocks of a set's twelve (4 to 12 frames, one block of several), and
    its first block alone as a single stream."""
    t = twelve_blocks(oracle)
    k = max(b for b in range(1, 13) if t["start"][b] <= 12)
    nf = int(t["start"][k])
    assert 4 <= nf <= 12 and max(t["nfr"][:k]) > 1
    off = np.concatenate([[0], np.cumsum(t["fbytes"])])
    n1 = int(t["start"][1])
    return dict(p=t["p"], bs=t["bs"], k=k, several=int(np.argmax(np.array(t["nfr"][:k]) > 1)), start=t["start"],
                blocks=(t["data"][:off[nf]], t["fbytes"][:nf], t["pcm"][:k * t["bs"]], t["first"][:k]),
                sequence=(t["data"][:off[n1]], t["fbytes"][:n1], t["pcm"][:t["bs"]], int(t["first"][0])))


def dev_twin(enc, torch, mode, stream, fb, pcm, arg, bs=None):
    """The _dev entry of `mode` on the same data: (summary, records)."""
    dev = torch.device("cuda")
    up = lambda a, dt: torch.from_numpy(np.array(a, dt).reshape(-1)).to(dev)        # (a writable copy)
    ds, dfb, dp = up(np.frombuffer(bytes(stream), np.uint8), np.uint8), up(fb, np.int32), up(pcm, np.int32)
    dsum = torch.full((4,), 99, dtype=torch.int64, device=dev)
    drec = torch.zeros((len(fb), 4), dtype=torch.int32, device=dev)
    ns = np.asarray(pcm).reshape(-1, enc.params.channels).shape[0]
    if mode == "sequence":
        enc.verify_frames_dev(ds, len(stream), dfb, len(fb), dp, ns, arg, dsum, drec)
    elif mode == "numbered":
        enc.verify_frames_dev(ds, len(stream), dfb, len(fb), dp, ns, 0, dsum, drec,
                              frame_numbers=up(np.asarray(arg, np.uint32).view(np.int32), np.int32))
    elif mode == "blocks":
        enc.verify_frames_blocks_dev(ds, len(stream), dfb, len(fb), dp, ns,
                                     up(np.asarray(arg, np.uint32).view(np.int32), np.int32), len(arg), bs, dsum, drec)
    else:
        numbers, sizes = arg
        src = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) * enc.params.channels
        vi = V.VerifyIn(ds.data_ptr(), len(stream), dfb.data_ptr(), len(fb), dp.data_ptr(), ns, 0)
        vo = V.VerifyOut(drec.data_ptr(), dsum.data_ptr())
        dn, dz, dsrc = up(np.asarray(numbers, np.uint32).view(np.int32), np.int32), up(sizes, np.int32), up(src, np.int64)
        assert enc.lib.fhip_verify_frames_ragged_dev(enc._h, C.byref(vi), dn.data_ptr(), dz.data_ptr(), dsrc.data_ptr(),
                                                     C.byref(vo)) == V.OK
    enc.sync()
    return dsum.cpu().numpy(), drec.cpu().numpy().reshape(-1)


def host(enc, mode, stream, fb, pcm, arg, bs=None):
    if mode == "sequence":
        return enc.verify_frames(stream, fb, pcm, arg)
    if mode == "numbered":
        return enc.verify_frames(stream, fb, pcm, frame_numbers=arg)
    if mode == "blocks":
        return enc.verify_frames_blocks(stream, fb, pcm, arg, bs)
    return enc.verify_frames_ragged(stream, fb, pcm, arg[0], arg[1])


def step(enc, torch, mode, inputs, bad_at, bs=None, bad_frame=None):
    """One mode, twice: the encoder's own output, then entry bad_at of its table off by one (sequence: first_sample
    one frame on).  bad_frame: the frame that entry's first frame is (the entry's own index unless blocks split)."""
    stream, fb, pcm, arg = inputs
    if mode == "ragged":
        arg = (arg, RAGGED_LENGTHS)
    n = len(fb)
    ok, recs, summ, err = host(enc, mode, stream, fb, pcm, arg, bs)
    print(mode, "good", list(summ), err)
    assert ok and list(summ) == [n, 0, -1, 0] and (recs["status"] == 0).all(), (mode, err)
    assert enc.last_verify_failure() is None
    dsum, drec = dev_twin(enc, torch, mode, stream, fb, pcm, arg, bs)
    assert np.array_equal(dsum, summ) and np.array_equal(drec, recs.view(np.int32).reshape(-1)), mode

    if mode == "sequence":
        bad, want, at = arg + (bs or BS), None, 0
    else:
        table = np.array(arg[0] if mode == "ragged" else arg, np.uint32)
        table[bad_at] += 1
        want, at = int(table[bad_at]), bad_at if bad_frame is None else bad_frame
        bad = (table, RAGGED_LENGTHS) if mode == "ragged" else table
    ok, recs, summ, err = host(enc, mode, stream, fb, pcm, bad, bs)
    print(mode, "bad", list(summ), err, enc.last_verify_failure())
    assert not ok and summ[2] == at and summ[3] == NUMBER and recs["status"][at] == NUMBER, (mode, list(summ), err)
    assert (recs["status"][:at] == 0).all()
    fsum, frec, fnum = enc.last_verify_failure()
    assert list(fsum) == list(summ) and frec["status"] == NUMBER and fnum == want, (mode, fnum, want)
    if want is not None:
        assert f"number {want}" in err, err
    dsum, drec = dev_twin(enc, torch, mode, stream, fb, pcm, bad, bs)
    assert np.array_equal(dsum, summ) and np.array_equal(drec, recs.view(np.int32).reshape(-1)), mode


def test_fixed_block_handle_takes_its_modes_in_turn(fixed, torch):
    with V.Encoder(fixed["p"], max_frames=16) as enc:
        for _ in range(2):
            step(enc, torch, "ragged", fixed["ragged"], 5)
            step(enc, torch, "numbered", fixed["numbered"], 3)
            step(enc, torch, "sequence", fixed["sequence"], None)
            step(enc, torch, "ragged", fixed["ragged"], 2)


def test_vbs_handle_takes_its_modes_in_turn(vbs, torch):
    b = vbs["several"]
    with V.Encoder(vbs["p"], max_frames=96) as enc:
        step(enc, torch, "blocks", vbs["blocks"], b, vbs["bs"], int(vbs["start"][b]))
        step(enc, torch, "sequence", vbs["sequence"], None, vbs["bs"])
        step(enc, torch, "blocks", vbs["blocks"], vbs["k"] - 1, vbs["bs"], int(vbs["start"][vbs["k"] - 1]))


def empty_call(enc, mode):
    """Zero frames (and zero blocks) through the raw entry, every table pointer non-null where the entry takes one."""
    s = np.full(4, 99, np.int64)
    num, sz = np.zeros(2, np.uint32), np.zeros(2, np.int32)
    vi = V.VerifyIn(None, 0, None, 0, None, 0, 0)
    vo = V.VerifyOut(None, s.ctypes.data)
    if mode == "sequence":
        rc = enc.lib.fhip_verify_frames(enc._h, C.byref(vi), C.byref(vo))
    elif mode == "numbered":
        rc = enc.lib.fhip_verify_frames_numbered(enc._h, C.byref(vi), num.ctypes.data, C.byref(vo))
    elif mode == "ragged":
        rc = enc.lib.fhip_verify_frames_ragged(enc._h, C.byref(vi), num.ctypes.data, sz.ctypes.data, C.byref(vo))
    else:
        rc = enc.lib.fhip_verify_frames_blocks(enc._h, C.byref(vi), None, 0, 128, C.byref(vo))
    return rc, list(s)


@pytest.mark.parametrize("handle,modes", [("fixed", ("sequence", "numbered", "ragged")), ("vbs", ("sequence", "blocks"))])
def test_empty_calls(handle, modes, torch):
    p = V.level_params(5, block_size=BS) if handle == "fixed" else V.level_params(10)
    n = p.block_size
    pcm = V.synth_pcm(2, n, 2, 16)
    with V.Encoder(p, max_frames=16) as enc:
        for m in modes:
            assert empty_call(enc, m) == (V.OK, [0, 0, -1, 0]), m
            assert enc.last_launches() == FRESH_HANDLE_LAUNCHES, m
        # behind an encode call the list stays that call's
        if handle == "fixed":
            enc.encode_subframes(pcm, n)
        else:
            enc.encode_blocks_vbs_packed_numbered(pcm, n, [0, n])
        for m in modes:
            assert empty_call(enc, m) == (V.OK, [0, 0, -1, 0]), m
            assert enc.last_launches() == BEHIND_AN_ENCODE[handle], m
            assert enc.last_verify_failure() is None
