"""The batches bench.py times, held to the CPU oracle bit for bit on every path.

The batch size chooses the kernels (k1_autocorr.hip: pick_autocorr, autocorr_does_lpc; narrow_rows_ok),
so the small batches of the other parity tests do not reach the instances the benchmark runs.  Each
case here is built the way bench.py builds it -- the device entry on a torch stream of its own, the
same flags, synth_pcm with the bench's first_frame, bench.workload() -- compared with the oracle over
the whole batch (tests/oracle_chunks.py: frame chunks on a thread pool), and its launch log
(fhip_last_launches) must show the path it claims to cover."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import bench
import flake_amd
import oracle_chunks as OC

pytestmark = pytest.mark.gpu

P = flake_amd.level_params
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_dev(p, nframes, first_frame=0, with_residual=False, pcm=None):
    """One batch as bench.py's step() queues it; returns host copies, the device bits and the log."""
    dev = torch.device("cuda", 0)
    n, ch = p.block_size, p.channels
    nsub = nframes * ch
    slot = flake_amd.rice_slot_bytes(p, n)
    if pcm is None:
        pcm = flake_amd.synth_pcm(nframes, n, ch, p.bits_per_sample, first_frame=first_frame)
    d_pcm = torch.from_numpy(pcm).to(dev)
    info = torch.zeros(nsub * flake_amd.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    bits = torch.zeros(nsub * slot, dtype=torch.uint8, device=dev)
    resid = torch.zeros((nframes, ch, n), dtype=torch.int32, device=dev) if with_residual else None
    with flake_amd.Encoder(p, max_frames=nframes) as enc:
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        enc.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            enc.encode_subframes_dev(d_pcm, nframes, n, info, residual=resid, rice_bits=bits, slot_bytes=slot)
        log = enc.last_launches()
        stream.synchronize()
    return dict(pcm=pcm, slot=slot, log=log, bits=bits.view(nsub, slot),
                info=np.frombuffer(info.cpu().numpy().tobytes(), flake_amd.INFO_DTYPE).copy(),
                residual=resid.cpu().numpy() if with_residual else None)


def check_dev(oracle, p, nframes, what, **kw):
    got = run_dev(p, nframes, **kw)
    OC.compare_batch(oracle, p, got["pcm"], p.block_size, got["info"], got["bits"], got["slot"],
                     residual=got["residual"], what=what)
    return got


# ---- reading a launch log -------------------------------------------------------------------------------
def entries(log, prefix):
    return [e for e in log if e.split()[0].startswith(prefix)]


def k1(log):
    """The batch's one K1 entry."""
    e = [x for x in log if x.startswith("k_autocorr")]
    assert len(e) == 1, log
    return e[0]


def flags(entry):
    return set(entry.split()[1:])


def assert_one_row_width(log):
    """16-bit rows are all or nothing: K0, a wave-typed K1, the search and K3 of a batch agree."""
    kinds = [e for e in log if e.startswith(("k_prepare", "k_autocorr_wt", "k_order_search", "k_encode"))]
    assert len({"narrow" in flags(e) for e in kinds}) <= 1, log


def pick_autocorr(nsub, n, max_order):
    """A transcription of k1_autocorr.hip's pick_autocorr: (kernel, split), kernel "wt" / "ps" / "cur"."""
    wave, ac_gmax, ps_gmax, tile, wt_sub, simds = 64, 12, 8, 128, 32, 1024
    nl2 = (max_order + 2) // 2
    g = max(1, min(wave // nl2, ac_gmax))
    waves_cur = (nsub + g - 1) // g
    ne, no = max_order // 2 + 1, (max_order + 1) // 2
    lps = 2 * ((ne + 2) // 3 + (no + 2) // 3)
    gp = min(wave // lps, ps_gmax)
    t_cur = float((waves_cur + 2 * simds - 1) // (2 * simds)) * (n * (41.0 if waves_cur > simds else 33.0) + 1000.0)
    t_ps = float(((nsub + gp - 1) // gp + simds - 1) // simds) * (0.5 * n * 39.0 + 1000.0) if gp >= 1 else 1e30
    t_wt, split = 1e30, 1
    if n % tile == 0:
        tiles = (nsub + wt_sub - 1) // wt_sub
        t_wt = float((tiles + 255) // 256) * (0.5 * n * max(4.8 * ((ne + 1) // 2), 23.0) + 8000.0)
        if 2 * tiles <= 256 and max_order >= 2:
            split = 2
            t_wt = 0.5 * n * max(4.8 * ((ne + 3) // 4), 14.0) + 8000.0
    k2 = 9000.0 if max_order <= 12 else 0.0
    kind = "wt" if (t_wt <= t_ps + k2 and t_wt <= t_cur + k2) else ("ps" if t_ps < t_cur else "cur")
    return kind, split


def assert_k1_choice(log, nsub, n, max_order):
    """The K1 entry is the kernel pick_autocorr's model chooses, split as it says, with K2 as its tail
    exactly where autocorr_does_lpc says (wave-typed, unsplit, order <= 12) and a K2 launch otherwise."""
    kind, split = pick_autocorr(nsub, n, max_order)
    e = k1(log)
    name = e.split()[0]
    if kind == "wt":
        assert name.startswith("k_autocorr_wt<") and f"split={split}" in flags(e), (kind, split, log)
        tail = split == 1 and max_order <= 12
    else:
        assert name == {"ps": "k_autocorr_ps", "cur": "k_autocorr"}[kind], (kind, log)
        assert not flags(e), log
        tail = False
    assert ("tail" in flags(e)) == tail, log
    assert len(entries(log, "k_lpc")) == (0 if tail else 1), log


# ---- configs[1], the headline -------------------------------------------------------------------------
HEADLINE_LOG = ["k_prepare_stereo<4,4,true> narrow", "k_autocorr_wt<3,false,8> split=1 tail narrow",
                "k_encode_pow2<16,256,0> narrow"]


@pytest.mark.parametrize("with_residual", [False, True], ids=["headline", "stage_a"])
def test_headline_4096_frames(oracle, with_residual):
    """bench.py's timed step: configs[1], 4096 frames, no residual and no samples (16-bit rows), K2 as
    K1's register tail; stage A (--with-residual) writes the int32 residual too, on the same path."""
    p, _, _ = bench.workload("configs[1]")
    got = check_dev(oracle, p, 4096, "configs[1] 4096", with_residual=with_residual)
    assert got["log"] == HEADLINE_LOG, got["log"]


def test_level5_est_4096_frames(oracle):
    """Level 5 as preset (order method EST: the Schur estimate in the tail) at the headline's size."""
    got = check_dev(oracle, P(5), 4096, "level 5 EST 4096")
    assert got["log"] == HEADLINE_LOG, got["log"]


def test_prepare_ahead_loop(oracle):
    """bench.py --ahead: two alternating 4096-frame batches (first frames 0 and 4096), the next batch's
    K0 hinted behind every step, one info / bits buffer throughout; every step's outputs are its
    batch's oracle outputs.  A hinted step queues no K0 of its own."""
    p, _, _ = bench.workload("configs[1]")
    n, ch, nfr = p.block_size, p.channels, 4096
    nsub, slot = nfr * ch, flake_amd.rice_slot_bytes(p, n)
    dev = torch.device("cuda", 0)
    pcms = [flake_amd.synth_pcm(nfr, n, ch, 16, first_frame=k * nfr) for k in range(2)]
    d_pcms = [torch.from_numpy(x).to(dev) for x in pcms]
    info = torch.zeros(nsub * flake_amd.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    bits = torch.zeros(nsub * slot, dtype=torch.uint8, device=dev)
    snaps, logs = [], []
    with flake_amd.Encoder(p, max_frames=nfr) as enc:
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        enc.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            for i in range(4):
                enc.encode_subframes_dev(d_pcms[i % 2], nfr, n, info, rice_bits=bits, slot_bytes=slot)
                logs.append(enc.last_launches())
                enc.prepare_ahead(d_pcms[(i + 1) % 2], nfr, n)
                logs.append(enc.last_launches())
                snaps.append((info.clone(), bits.clone()))
        stream.synchronize()
    assert logs[0] == HEADLINE_LOG, logs[0]
    for i in range(1, 4):
        assert logs[2 * i] == HEADLINE_LOG[1:], (i, logs[2 * i])         # K0 ran ahead
    for i in range(4):
        assert logs[2 * i + 1] == HEADLINE_LOG[:1], (i, logs[2 * i + 1])
    host = [(np.frombuffer(a.cpu().numpy().tobytes(), flake_amd.INFO_DTYPE).copy(), b.view(nsub, slot))
            for a, b in snaps]
    for i in range(2):
        OC.compare_batch(oracle, p, pcms[i], n, host[i][0], host[i][1], slot, what=f"--ahead step {i}")
    for i in range(2, 4):                    # the same batches again: byte for byte what steps 0 / 1 wrote
        assert host[i][0].tobytes() == host[i - 2][0].tobytes(), i
        nb = (np.maximum(host[i][0]["rice_nbits"].astype(np.int64), 0) + 7) // 8
        w = int(nb.max())
        a, b = host[i][1][:, :w].cpu().numpy(), host[i - 2][1][:, :w].cpu().numpy()
        assert not ((a != b) & (np.arange(w)[None, :] < nb[:, None])).any(), i


# ---- bench.py other_configs and small_batch, at their sizes ---------------------------------------------
OTHER = {
    "configs2": (lambda: P(5, bits_per_sample=24, sample_rate=96000, order_method=flake_amd.OM_SEARCH,
                           max_prediction_order=32, max_partition_order=8), 4096),
    "configs3": (lambda: bench.workload("configs[3]")[0], 4096),
    "configs0_gpu": (lambda: P(2, channels=1, block_size=4096), 8192),
    "level8": (lambda: P(8), 4096),
    "level2": (lambda: P(2), 4096 * 4096 // 1152),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_configs_at_bench_size(oracle, name):
    make, nframes = OTHER[name]
    p = make()
    got = check_dev(oracle, p, nframes, f"{name} at {nframes} frames")
    log = got["log"]
    assert_one_row_width(log)
    assert len(entries(log, "k_prepare")) == 1 and len(entries(log, "k_encode")) == 1, log
    if p.prediction_type == flake_amd.PRED_LEVINSON:
        assert_k1_choice(log, nframes * p.channels, p.block_size, p.max_prediction_order)
        searched = p.order_method >= 2
        assert len(entries(log, "k_order_search")) == (1 if searched else 0), log
    else:
        assert not entries(log, "k_autocorr") and not entries(log, "k_lpc"), log


@pytest.mark.parametrize("workload,nframes", [("configs[1]", 512), ("configs[1]", 1024), ("configs[1]", 2048),
                                              ("configs[3]", 512), ("configs[3]", 1024)])
def test_small_batches(oracle, workload, nframes):
    """bench.py small_batch: the shards of a split batch -- K1's lags over two workgroups per tile and
    K2 as a launch of its own where the batch has at most 128 tiles of 32 subframes."""
    p, _, _ = bench.workload(workload)
    got = check_dev(oracle, p, nframes, f"{workload} at {nframes} frames")
    assert_k1_choice(got["log"], nframes * p.channels, p.block_size, p.max_prediction_order)
    assert_one_row_width(got["log"])


# ---- both sides of every switch of pick_autocorr --------------------------------------------------------
def _switches(n, max_order, ch, limit=20000):
    out, prev = [], None
    for f in range(1, limit + 1):
        c = pick_autocorr(f * ch, n, max_order)
        if prev is not None and c != prev:
            out.append(f - 1)
        prev = c
    return out


# (n, max order, channels) -> the last batch size before each switch, from the transcription above
BOUNDARIES = {(4096, 8, 2): [2048], (4096, 12, 2): [2048], (512, 8, 2): [2048, 4096, 6144, 8192, 12288, 16384],
              (1024, 12, 2): [2048, 8192, 9216, 16384, 18432], (1152, 8, 2): [2048, 8192, 12288, 16384],
              (2048, 8, 2): [2048, 8192, 12288], (4096, 8, 1): [4096]}
BOUNDARY_CASES = [(n, mo, ch, f) for (n, mo, ch), fs in BOUNDARIES.items() for f in fs]


def test_boundary_table_is_the_transcription():
    assert {k: _switches(*k) for k in BOUNDARIES} == BOUNDARIES


@pytest.mark.parametrize("n,max_order,ch,frames", BOUNDARY_CASES,
                         ids=[f"n{n}_o{mo}_ch{ch}_{f}" for n, mo, ch, f in BOUNDARY_CASES])
def test_pick_autocorr_boundary(oracle, n, max_order, ch, frames):
    """Batch sizes `frames` and `frames + 1` take different K1 instances (or lag splits); each is the
    oracle's bit for bit, and each log is the one the kernel choice's model predicts."""
    p = P(5, channels=ch, block_size=n, order_method=flake_amd.OM_MAX, max_prediction_order=max_order)
    logs = []
    for f in (frames, frames + 1):
        got = check_dev(oracle, p, f, f"n {n} order {max_order} ch {ch}: {f} frames",
                        first_frame=3 * f)
        assert_k1_choice(got["log"], f * ch, n, max_order)
        assert_one_row_width(got["log"])
        logs.append(k1(got["log"]))
    assert logs[0] != logs[1], logs


# ---- FHIP_OVERLAP=1: two half-batches on two internal streams --------------------------------------------
def test_overlap_split_batch_subprocess():
    """FHIP_OVERLAP=1 (read once per process: a child) cuts a batch of >= 512 frames into two halves on
    the handle's two internal streams (api.hip run_pipeline).  Each half is a 2048-frame range: lag-split
    K1 and K2 of its own; the second half's subframes start mid-workspace.  The whole batch against the
    oracle."""
    code = textwrap.dedent("""
        import sys, json
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import bench, flake_amd, oracle_chunks as OC
        from oraclelib import Oracle
        p, _, _ = bench.workload("configs[1]")
        n, nfr = p.block_size, 4096
        pcm = flake_amd.synth_pcm(nfr, n, 2, 16)
        with flake_amd.Encoder(p, max_frames=nfr) as enc:
            got = enc.encode_subframes(pcm, n)
            log = enc.last_launches()
        OC.compare_batch(Oracle(), p, pcm, n, got["info"], got["rice_bits"], got["slot_bytes"],
                         residual=got["residual"], what="FHIP_OVERLAP=1")
        print("LOG " + json.dumps(log))
        print("overlap ok")
    """ % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, FHIP_OVERLAP="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "overlap ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    log = json.loads([x for x in r.stdout.splitlines() if x.startswith("LOG ")][0][4:])
    half = ["k_prepare_stereo<4,4,true> narrow", "k_autocorr_wt<2,false,0> split=2 narrow", "k_lpc_reg<8>",
            "k_encode_pow2<16,256,0> narrow"]
    assert log == half + half, log


# ---- configs[4]: variable block size through the device entry ---------------------------------------------
def vbs_bench_pcm(nblocks, n):
    pcm = flake_amd.synth_pcm(nblocks, n, 2, 16)
    pcm[::3, n // 2:, :] //= 16            # bench.py vbs_case: a transient in every third block
    return pcm


VBS_BIG = os.environ.get("FLAKE_BENCH_VBS_BIG", "1") != "0"


@pytest.mark.parametrize("level,nblocks", [(10, 1024), (12, 1024),
                                           pytest.param(10, 8192, marks=pytest.mark.skipif(
                                               not VBS_BIG, reason="FLAKE_BENCH_VBS_BIG=0"))])
def test_vbs_dev_bench_size(oracle, level, nblocks):
    """bench.py vbs_case: the whole packed stream and every block's byte count equal the oracle's."""
    p = P(level)
    n = p.block_size
    pcm = vbs_bench_pcm(nblocks, n)
    dev = torch.device("cuda", 0)
    cap = pcm.size * 5
    d_pcm = torch.from_numpy(pcm).to(dev)
    packed = torch.zeros(cap, dtype=torch.uint8, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    bbytes = torch.zeros(nblocks, dtype=torch.int32, device=dev)
    with flake_amd.Encoder(p, max_frames=8 * nblocks) as enc:
        torch.cuda.synchronize(dev)
        stream = torch.cuda.Stream(dev)
        enc.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            enc.encode_blocks_vbs_dev(d_pcm, nblocks, n, packed, cap, totals, block_bytes=bbytes)
        log = enc.last_launches()
        stream.synchronize()
    nfr, nbytes, _, cut = (int(v) for v in totals.cpu().numpy())
    assert cut == 0 and nfr > nblocks, (nfr, cut)
    exp, esizes = OC.oracle_blocks(oracle, p, pcm, n)
    msg = OC.stream_mismatch(packed[:nbytes].cpu().numpy(), exp, bbytes.cpu().numpy(), esizes)
    assert msg is None, f"level {level}, {nblocks} blocks: {msg}"
    assert log[:2] == ["k_vbs_split", "k_vbs_plan"] and log[-2:] == ["k_pack_frames_perm", "k_vbs_block_bytes"], log
    e = k1(log)
    assert e.startswith("k_autocorr_wt<") and ("tail" in flags(e)) == (p.max_prediction_order <= 12), log
    assert len(entries(log, "k_lpc")) == (0 if p.max_prediction_order <= 12 else 1), log
