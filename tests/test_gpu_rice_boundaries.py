"""Every Rice-parameter site held to the oracle at boundary sums (tests/ricecases.py): frames whose partition sums, thread
sums and first-partition counts sit exactly where the closed forms of find_optimal_rice_param (device_util.h) and the
width switches on the way to them change branch, through the entry of each site; the launch log must name the kernel
instance a case was built for.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import flake_amd
import ricecases as R
from parity import assert_bits_equal, assert_info_equal, assert_residual_equal

pytestmark = pytest.mark.gpu

GOLDEN = R.__file__.replace("ricecases.py", "golden/ref_rice_cases.npz")
CFGS = {}
for _key in R.groups():
    CFGS.setdefault(_key[0], []).append(_key)
NAMES = sorted(CFGS)
SEARCH_NAMES = [k for k in NAMES if k.startswith("S4")]
_LOGS = {}                                      # group key -> the launch log of its encode call


def recorded_answers():
    if "gold" not in _LOGS:
        _LOGS["gold"] = R.unpack_answers(np.load(GOLDEN))          # (read once for the module)
    return _LOGS["gold"]


def run_group(oracle, key):
    """one group (one parameter set) through fhip_encode_subframes, held to the oracle; returns the launch log"""
    if key in _LOGS:
        return _LOGS[key]
    p, pcm, exp = R.expected(oracle, key)
    n = pcm.shape[1]
    with flake_amd.Encoder(p, max_frames=pcm.shape[0]) as enc:
        got = enc.encode_subframes(pcm, n)
        log = enc.last_launches()
    what = f"{key[0]} pinned {key[1]}"
    assert got["slot_bytes"] == exp["rice_bits"].shape[1]
    assert_info_equal(got["info"], exp["info"], what)
    assert_residual_equal(got["residual"], exp["residual"], exp["info"], what)
    assert_bits_equal(got["rice_bits"], exp["rice_bits"], exp["info"], what)
    cfg = R.groups()[key][0].cfg
    assert any(name.startswith(cfg.launch_for(key[1])) for name in log), (what, cfg.launch_for(key[1]), log)
    _LOGS[key] = log
    return log


@pytest.mark.parametrize("name", NAMES)
def test_site_entry(oracle, name):
    """S1 .. S4, S7's long block: every group of the configuration (the free search and each pinned level)"""
    for key in CFGS[name]:
        log = run_group(oracle, key)
        cfg = R.groups()[key][0].cfg
        if cfg.site == "S4":                     # the search kernel names the order; the lean / wide-row instance encodes it
            mode = 3 if cfg.maxorder > 8 else 0
            assert any(nm.startswith("k_encode_pow2<") and nm.split(">")[0].endswith(f",{mode}") for nm in log), log


def test_launch_logs_cover_the_site_list(oracle):
    want = {cfg.launch for cfg in R.site_configs()} | {cfg.launch for cfg in R.first_partition_configs()}
    seen = set()
    for name in NAMES:
        key = (name, None) if (name, None) in CFGS[name] else CFGS[name][0]           # (already run: from the cache)
        seen.update(nm.replace(" narrow", "") for nm in run_group(oracle, key))
    assert want <= seen, sorted(want - seen)
    for inst in ("k_encode_pow2<16,256,0>", "k_encode_pow2<16,256,3>", "k_encode_pow2<9,256,2>", "k_encode_pow2<16,256,1>",
                 "k_order_search<16,256,4,false>", "k_order_search<16,256,4,true>", "k_encode_big"):
        assert inst in seen, inst


@pytest.mark.parametrize("name", SEARCH_NAMES)
def test_order_search_table(oracle, name):
    """S4 through fhip_order_search_bits: every visited entry of the bits[] table (optimize.c:201-261), not only the winner"""
    for key in CFGS[name]:
        lst = R.groups()[key]
        p, cfg = lst[0].params(), lst[0].cfg
        blocks = np.stack([c.samples() for c in lst])
        obits = np.full(len(lst), cfg.bps, np.int32)
        with flake_amd.Encoder(p, max_frames=len(lst)) as enc:
            table = enc.order_search_bits(blocks, obits)          # (a stage entry: it keeps no launch log)
        hi, visited = p.max_prediction_order, 0
        for s, c in enumerate(lst):
            coefs, shift, _ = oracle.lpc_calc_coefs(blocks[s], hi, p.lpc_precision, p.order_method)
            for o in range(1, hi + 1):
                if table[s, o - 1] == 0xFFFFFFFF:
                    continue
                res = oracle.residual_lpc(blocks[s], o, coefs[o - 1], int(shift[o - 1]))
                bits, _ = oracle.subframe_bits(res, p.min_partition_order, p.max_partition_order, o, cfg.bps,
                                               p.lpc_precision, True)
                assert int(table[s, o - 1]) == int(bits) & 0xFFFFFFFF, (c.name, o, table[s, o - 1], bits)
                visited += 1
            if p.order_method == flake_amd.OM_SEARCH:
                assert (table[s, :hi] != 0xFFFFFFFF).all(), c.name
        assert visited >= 2 * len(lst)


@pytest.mark.parametrize("name", NAMES)
def test_generic_search_on_given_residuals(oracle, name):
    """S7: fhip_calc_rice_params (the generic search: the scan itself) on every case's residuals, against the answers the
    compiled rice.c gave (tests/golden/ref_rice_cases.npz) and the oracle's Rice bytes"""
    gold = recorded_answers()
    for key in CFGS[name]:
        p, pcm, exp = R.expected(oracle, key)
        lst, ch, n = R.groups()[key], p.channels, pcm.shape[1]
        calls = {}
        for i, c in enumerate(lst):
            calls.setdefault(R.rice_call(p, exp["info"][i * ch]), []).append(i)
        slot = exp["rice_bits"].shape[1]
        with flake_amd.Encoder(p, max_frames=len(lst)) as enc:
            for (lpc, pmin, pmax, order, bps, _), idx in calls.items():
                res = np.ascontiguousarray(exp["residual"][idx, 0])
                out = enc.calc_rice_params(res, order, lpc, bps, pmin, pmax, slot_bytes=slot)
                sub = exp["info"][[i * ch for i in idx]]
                for q, i in enumerate(idx):
                    info = out["info"][q]
                    por = int(info["porder"])
                    got = (int(info["est_bits"]), int(info["rice_method"]), por, [int(v) for v in info["rparams"][:1 << por]])
                    assert got == gold[lst[i].name], (lst[i].name, got[:3], gold[lst[i].name][:3])
                assert (out["info"]["rice_nbits"] == sub["rice_nbits"]).all(), name
                assert_bits_equal(out["rice_bits"], exp["rice_bits"][[i * ch for i in idx]], sub, name)


STEREO = sorted({(c.n, c.bps) for c in R.stereo_cases()})


@pytest.mark.parametrize("n,bps", STEREO)
def test_stereo_estimate(oracle, n, bps):
    """S6 / F8: K0's estimate (encode.c:598-643) with the left channel's 2 * sum at the closed form's limits: the channel
    mode, the prepared samples and everything behind them"""
    lst = [c for c in R.stereo_cases() if (c.n, c.bps) == (n, bps)]
    p = flake_amd.level_params(5, channels=2, bits_per_sample=bps, block_size=n)
    pcm = np.stack([c.pcm() for c in lst])
    with flake_amd.Encoder(p, max_frames=len(lst)) as enc:
        got = enc.encode_subframes(pcm, n, want_samples=True)
        log = enc.last_launches()
    exp = oracle.encode_subframes_batch(p, pcm, n, slot_bytes=got["slot_bytes"])
    assert any(nm.startswith("k_prepare_stereo<") for nm in log), log
    modes = set()
    for f, c in enumerate(lst):
        _, smp, _ = oracle.prepare_frame(p, pcm[f], n)
        assert (got["samples"][f] == smp).all(), c.name
        modes.add(int(exp["info"]["ch_mode"][2 * f]))
    assert len(modes) >= 2, modes
    assert_info_equal(got["info"], exp["info"], f"stereo n{n} {bps}")
    assert_residual_equal(got["residual"], exp["residual"], exp["info"], f"stereo n{n} {bps}")
    assert_bits_equal(got["rice_bits"], exp["rice_bits"], exp["info"], f"stereo n{n} {bps}")


def vbs_stream(oracle, decoder, p, pcm, n):
    """one variable-block-size batch on the device, held to the oracle's flake_encode_frame() loop byte for byte and
    decoded back; returns the launch log"""
    from test_host_frames import oracle_stream
    nblocks, ch = pcm.shape[0], p.channels
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm, np.int32)).to(dev)
    cap = pcm.size * 5 + 4096
    packed = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    with flake_amd.Encoder(p, max_frames=8 * nblocks) as enc:
        enc.encode_blocks_vbs_dev(d_pcm, nblocks, n, packed, cap, totals)
        enc.sync()
        log = enc.last_launches()
    nfr, nbytes, _, cut = (int(v) for v in totals.cpu().numpy())
    exp, _ = oracle_stream(oracle, p, pcm.reshape(-1, ch), n)
    out = packed.cpu().numpy()
    assert cut == 0 and nbytes == exp.size and out[:nbytes].tobytes() == exp.tobytes()
    assert (out[cap:] == 0xA5).all()
    back, _ = decoder.decode(out[:nbytes], ch, p.bits_per_sample, nblocks * n)
    assert (back == pcm.reshape(-1, ch)).all()
    return log


@pytest.mark.parametrize("level", [9, 10])
def test_vbs_batch_of_table_frames(oracle, decoder, level):
    """S5: whole frames of the table as the blocks of one variable-block-size batch, small enough for the one-launch
    path (k_order_search_bins / k_encode_bins).  The splitter cuts where the samples tell it to; what it leaves on a
    limit is read back: where it cuts a first piece of 512 samples off a frame pinned to level 8, level 5 of that
    piece's search has partitions 1 .. 31 of the frame's own sixteen samples each, and their sums stay on F2's limits."""
    mine = [c for c in R.cases() if c.cfg.name == "S1-n4096-o8-2x16-p8" and c.family in ("F1", "F2")]
    lst = [c for c in mine if c.pin in (8, 6)] + [c for c in mine if c.pin == 3][:4]
    assert len(lst) == 8
    pcm = np.stack([c.pcm() for c in lst])
    p = flake_amd.level_params(level, block_size=4096)
    assert p.channels == 2 and p.bits_per_sample == 16
    on_limit = 0
    for b, c in enumerate(lst):
        sizes = oracle.vbs_split(pcm[b], 2, 4096)[1]
        if c.family != "F2" or c.pin != 8 or int(sizes[0]) != 512:
            continue
        piece = oracle.encode_subframes_batch(p, pcm[b:b + 1, :512], 512)
        info, res = piece["info"][0], piece["residual"][0, 0]
        order = int(info["order"])
        assert info["type"] == 32 and not info["coefs"].any() and (res[order:] == pcm[b, order:512, 0]).all(), c.name
        assert p.min_partition_order <= 5 <= R.limit_porder(p.max_partition_order, 512, order)
        sums = R.level_sums(res, order, 5, 5)[5]
        for nd in c.prop["nodes"]:
            if nd["level"] == 8 and 1 <= nd["node"] < 32 and nd["tag"].startswith("k"):
                assert sums[nd["node"]] == nd["sum"] and nd["cnt"] == 16, (c.name, nd)
                k = int(nd["tag"][1:].rstrip("atlohic+-"))
                assert nd["sum"] - 8 in [v for v, _ in R._f2_values(16, k)], (c.name, nd)
                on_limit += 1
    assert on_limit >= 20, on_limit
    log = vbs_stream(oracle, decoder, p, pcm, 4096)
    assert any(nm.startswith("k_encode_bins<") for nm in log), log
    assert any(nm.startswith("k_order_search_bins<") for nm in log), log


def test_vbs_batch_stereo_two_pass(oracle, decoder):
    """S6's second body: blocks of 8192 stereo samples built as F8's cases; pieces above 4096 samples take K0's
    two-pass body inside k_prepare_stereo_bins<8>"""
    lst = R.stereo_cases(((8192, 16),))
    pcm = np.stack([c.pcm() for c in lst])
    p = flake_amd.level_params(11)
    assert (p.block_size, p.channels, p.bits_per_sample) == (8192, 2, 16)
    longest = [int(oracle.vbs_split(b, 2, 8192)[1].max()) for b in pcm]
    assert sum(v > 4096 for v in longest) >= len(lst) // 2 and 8192 in longest
    log = vbs_stream(oracle, decoder, p, pcm, 8192)
    assert any(nm.startswith("k_prepare_stereo_bins<8>") for nm in log), log
