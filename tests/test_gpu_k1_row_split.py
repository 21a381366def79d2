"""K1's producer row split (k1_autocorr.hip: wt_split_of) against the CPU oracle, bit for bit, at the smallest shapes
at which an uneven split can go wrong.

Every case encodes through fhip_encode_subframes_dev (the C ABI) and asks for K1's autoc beside the records.  autoc
is compared as uint64 images with the oracle's window + autocorrelation of the oracle's own prepared channels; what
K2 made of it (the quantised row K3 used: coefficients, shift and order in the records) and the Rice bytes are
held to the oracle over the whole batch (tests/oracle_chunks.py).  Each case runs again under FHIP_WT_TILE=128
(read per launch): the 128 form must give the same autoc images, records and bytes as the long form.

The unsplit instance (the one with a split of its own at max order 8) needs more than 128 workgroups of 32
subframes, hence 2081 stereo frames (4162 subframes: the last workgroup holds two live rows) or 4129 mono ones (one
live row: every producer but the first stages clamped rows).  The shapes the lag-split launch takes (33 subframes,
16 frames) are held to the same checks.  Rows are stored as int16 ("narrow" in the launch log) only where K3's
geometry takes them: of these shapes at n = 512, which is where a producer reads its rows' width flags.  There the
last workgroup's two live rows leave three producers with nothing but clamped rows."""
import numpy as np
import pytest
import torch

import flake_amd
import oracle_chunks as OC

pytestmark = pytest.mark.gpu

P = flake_amd.level_params


def params(n, mo=8, ch=2):
    return P(5, channels=ch, block_size=n, order_method=flake_amd.OM_MAX, max_prediction_order=mo)


def antiphase_pcm(nframes, n, ch=2):
    """synth_pcm with every fifth frame replaced by loud channels in anti-phase: mid is silence there and the side
    channel needs 17 bits, so a producer's rows mix int16 and int32 storage (frames 0, 5, 10, 15 of a workgroup's 16:
    rows 1, 11, 21, 31 -- an uneven split moves which producer meets them)."""
    pcm = flake_amd.synth_pcm(nframes, n, 2, 16)
    loud = np.empty(pcm[::5, :, 0].shape, dtype=np.int32)
    loud[:, ::2] = 30000
    loud[:, 1::2] = -30000 + (np.arange(n // 2) % 97)
    pcm[::5, :, 0] = loud
    pcm[::5, :, 1] = -loud
    return pcm


def zero_ends_pcm(nframes, n, ch=2):
    """Every third frame starts with 128 zeros (the head and the first pass see nothing but zeros), the frames after
    those end with 128 zeros (the last pass stages nothing but zeros)."""
    pcm = flake_amd.synth_pcm(nframes, n, ch, 16)
    pcm[0::3, :128, :] = 0
    pcm[1::3, n - 128:, :] = 0
    return pcm


UNSPLIT8 = "k_autocorr_wt<3,false,8> split=1 tail"
# id -> (n, max order, channels, frames, form, K1 log entry, pcm maker or None)
CASES = {
    "a_n256_tile0_is_last": (256, 8, 2, 2081, 256, UNSPLIT8, None),
    "b_n512": (512, 8, 2, 2081, 256, UNSPLIT8 + " narrow", None),
    "c_n384_128_form": (384, 8, 2, 2081, 128, UNSPLIT8, None),
    "d_n256_order12": (256, 12, 2, 2081, 256, "k_autocorr_wt<4,false,12> split=1 tail", None),
    "e_n512_order12": (512, 12, 2, 2081, 256, "k_autocorr_wt<4,false,12> split=1 tail narrow", None),
    "f_33_subframes": (512, 8, 1, 33, 256, "split=2", None),
    "g_one_live_row_in_last_workgroup": (256, 8, 1, 4129, 256, UNSPLIT8, None),
    "h_16_frames_17bit_side": (512, 8, 2, 16, 256, "split=2", antiphase_pcm),
    "i_17bit_side_unsplit": (512, 8, 2, 2081, 256, UNSPLIT8 + " narrow", antiphase_pcm),
    "j_zero_first_and_last_pass_n512": (512, 8, 2, 2081, 256, UNSPLIT8 + " narrow", zero_ends_pcm),
    "k_zero_first_and_last_pass_n256": (256, 8, 2, 2081, 256, UNSPLIT8, zero_ends_pcm),
    "l_zero_ends_order12": (512, 12, 2, 2081, 256, "k_autocorr_wt<4,false,12> split=1 tail", zero_ends_pcm),
}


def run_dev(p, nframes, pcm):
    dev = torch.device("cuda", 0)
    n, ch = p.block_size, p.channels
    nsub = nframes * ch
    slot = flake_amd.rice_slot_bytes(p, n)
    d_pcm = torch.from_numpy(pcm).to(dev)
    info = torch.zeros(nsub * flake_amd.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    bits = torch.zeros(nsub * slot, dtype=torch.uint8, device=dev)
    autoc = torch.zeros(nsub * flake_amd.MAX_LAGS, dtype=torch.float64, device=dev)
    with flake_amd.Encoder(p, max_frames=nframes) as enc:
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        enc.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            enc.encode_subframes_dev(d_pcm, nframes, n, info, rice_bits=bits, slot_bytes=slot, autoc=autoc)
        log = enc.last_launches()
        stream.synchronize()
    return dict(slot=slot, log=log, bits=bits.view(nsub, slot),
                autoc=autoc.cpu().numpy().view(np.uint64).reshape(nsub, flake_amd.MAX_LAGS).copy(),
                info=np.frombuffer(info.cpu().numpy().tobytes(), flake_amd.INFO_DTYPE).copy())


def oracle_autoc_bits(oracle, p, pcm, mo):
    """uint64 images of lags 0..mo of the oracle's autocorrelation of every prepared channel."""
    n, ch = p.block_size, p.channels
    out = np.zeros((pcm.shape[0] * ch, mo + 1), dtype=np.uint64)
    for f in range(pcm.shape[0]):
        _, smp, _ = oracle.prepare_frame(p, pcm[f], n)
        for c in range(ch):
            out[f * ch + c] = oracle.window_autocorr(smp[c], mo)[:mo + 1].view(np.uint64)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_row_split_case(oracle, monkeypatch, case):
    n, mo, ch, nframes, form, k1_entry, make_pcm = CASES[case]
    p = params(n, mo, ch)
    nsub = nframes * ch
    tile = flake_amd.load_library().fhip_autocorr_tile
    monkeypatch.delenv("FHIP_WT_TILE", raising=False)
    assert tile(nsub, n, mo) == form, (case, tile(nsub, n, mo))
    pcm = make_pcm(nframes, n, ch) if make_pcm else flake_amd.synth_pcm(nframes, n, ch, 16)

    got = run_dev(p, nframes, pcm)
    k1 = [e for e in got["log"] if e.startswith("k_autocorr")]
    assert len(k1) == 1 and k1_entry in k1[0], got["log"]
    exp_ac = oracle_autoc_bits(oracle, p, pcm, mo)
    bad = np.nonzero((got["autoc"][:, :mo + 1] != exp_ac).any(axis=1))[0]
    assert bad.size == 0, (case, "autoc", bad.size, bad[:8], got["autoc"][bad[0], :mo + 1], exp_ac[bad[0]])
    OC.compare_batch(oracle, p, pcm, n, got["info"], got["bits"], got["slot"], what=case)
    if make_pcm is antiphase_pcm:
        side = np.abs(pcm[::5, :, 0].astype(np.int64) - pcm[::5, :, 1]).max()
        assert side >= 1 << 15
        modes = got["info"]["ch_mode"].reshape(nframes, 2)[:, 0]
        assert (modes[::5] != flake_amd.CH_LEFT_RIGHT).all(), np.unique(modes[::5])

    monkeypatch.setenv("FHIP_WT_TILE", "128")
    assert tile(nsub, n, mo) == 128
    old = run_dev(p, nframes, pcm)
    assert old["log"] == got["log"]
    assert np.array_equal(old["autoc"][:, :mo + 1], got["autoc"][:, :mo + 1]), (case, "autoc, 128 form")
    assert old["info"].tobytes() == got["info"].tobytes(), case
    nb = (np.maximum(got["info"]["rice_nbits"].astype(np.int64), 0) + 7) // 8
    w = int(nb.max())
    a, b = got["bits"][:, :w].cpu().numpy(), old["bits"][:, :w].cpu().numpy()
    assert not ((a != b) & (np.arange(w)[None, :] < nb[:, None])).any(), case
