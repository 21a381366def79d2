"""K1's long-tile form (k_autocorr_wtl: 256 positions per hand-over, two LDS buffers, the halo carried in the
producers' registers) against the CPU oracle, and against the 128 form of the same build.

Every case asserts through fhip_autocorr_tile which form it runs, encodes through encode_subframes_dev,
is held to the oracle over the whole batch (tests/oracle_chunks.py), and runs again under FHIP_WT_TILE=128
(read per launch): records and Rice bytes of the two runs must be identical.  The unsplit form needs more than
128 workgroups of 32 subframes, hence 2081 stereo frames (4162 subframes: the last workgroup holds two live
ones) of short blocks."""
import numpy as np
import pytest
import torch

import flake_amd
import oracle_chunks as OC

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
MAX8 = dict(order_method=flake_amd.OM_MAX)


def stereo16(n, **kw):
    return P(5, block_size=n, **MAX8, **kw)


def antiphase_pcm(nframes, n):
    """synth_pcm with every fifth frame replaced by loud channels in anti-phase: mid is silence there and the side
    channel needs 17 bits, so a 16-bit batch carries int32 rows next to int16 ones."""
    pcm = flake_amd.synth_pcm(nframes, n, 2, 16)
    loud = np.empty(pcm[::5, :, 0].shape, dtype=np.int32)
    loud[:, ::2] = 30000
    loud[:, 1::2] = -30000 + (np.arange(n // 2) % 97)
    pcm[::5, :, 0] = loud
    pcm[::5, :, 1] = -loud
    return pcm


# id -> (params, frames, form, K1 log entry or None, pcm maker or None)
CASES = {
    "a_n256_one_tile": (lambda: stereo16(256), 2081, 256, None, None),
    "b_n512_one_handover": (lambda: stereo16(512), 2081, 256, None, None),
    "c_n768_buffer0_reused": (lambda: stereo16(768), 2081, 256, None, None),
    "d_n1024_two_ring_turns": (lambda: stereo16(1024), 2081, 256, None, None),
    "e_n384_stays_128": (lambda: stereo16(384), 2081, 128, None, None),
    "f_lag_split_8_frames": (lambda: stereo16(768), 8, 256, "split=2", None),
    "g_8ch_24bit_order12": (lambda: P(5, channels=8, bits_per_sample=24, block_size=512, max_prediction_order=12,
                                      **MAX8), 521, 256, "k_autocorr_wt<4,false,12> split=1 tail", None),
    "h_24bit_order32": (lambda: P(5, bits_per_sample=24, block_size=512, max_prediction_order=32, **MAX8),
                        2081, 256, "k_autocorr_wt<9,false,0> split=1", None),
    "i_antiphase_17bit_side": (lambda: stereo16(2048), 2081, 256, "k_autocorr_wt<3,false,8> split=1 tail narrow",
                               antiphase_pcm),
}


def run_dev(p, nframes, pcm):
    dev = torch.device("cuda", 0)
    n, ch = p.block_size, p.channels
    nsub = nframes * ch
    slot = flake_amd.rice_slot_bytes(p, n)
    d_pcm = torch.from_numpy(pcm).to(dev)
    info = torch.zeros(nsub * flake_amd.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    bits = torch.zeros(nsub * slot, dtype=torch.uint8, device=dev)
    with flake_amd.Encoder(p, max_frames=nframes) as enc:
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        enc.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            enc.encode_subframes_dev(d_pcm, nframes, n, info, rice_bits=bits, slot_bytes=slot)
        log = enc.last_launches()
        stream.synchronize()
    return dict(slot=slot, log=log, bits=bits.view(nsub, slot),
                info=np.frombuffer(info.cpu().numpy().tobytes(), flake_amd.INFO_DTYPE).copy())


@pytest.mark.parametrize("case", list(CASES))
def test_long_tile_case(oracle, monkeypatch, case):
    make, nframes, form, k1_entry, make_pcm = CASES[case]
    p = make()
    n, nsub, mo = p.block_size, nframes * p.channels, p.max_prediction_order
    tile = flake_amd.load_library().fhip_autocorr_tile
    monkeypatch.delenv("FHIP_WT_TILE", raising=False)
    assert tile(nsub, n, mo) == form, (case, tile(nsub, n, mo))
    pcm = make_pcm(nframes, n) if make_pcm else flake_amd.synth_pcm(nframes, n, p.channels, p.bits_per_sample)

    got = run_dev(p, nframes, pcm)
    k1 = [e for e in got["log"] if e.startswith("k_autocorr")]
    assert len(k1) == 1 and k1[0].startswith("k_autocorr_wt<"), got["log"]
    if k1_entry:
        assert k1_entry in k1[0], got["log"]
    OC.compare_batch(oracle, p, pcm, n, got["info"], got["bits"], got["slot"], what=case)
    if make_pcm is antiphase_pcm:
        # the loud frames took a side channel wider than 16 bits, their neighbours did not
        side = np.abs(pcm[::5, :, 0].astype(np.int64) - pcm[::5, :, 1]).max()
        assert side >= 1 << 15
        modes = got["info"]["ch_mode"].reshape(nframes, 2)[:, 0]
        assert (modes[::5] != flake_amd.CH_LEFT_RIGHT).all(), np.unique(modes[::5])

    monkeypatch.setenv("FHIP_WT_TILE", "128")
    assert tile(nsub, n, mo) == 128
    old = run_dev(p, nframes, pcm)
    assert old["log"] == got["log"]
    assert old["info"].tobytes() == got["info"].tobytes(), case
    nb = (np.maximum(got["info"]["rice_nbits"].astype(np.int64), 0) + 7) // 8
    w = int(nb.max())
    a, b = got["bits"][:, :w].cpu().numpy(), old["bits"][:, :w].cpu().numpy()
    assert not ((a != b) & (np.arange(w)[None, :] < nb[:, None])).any(), case
