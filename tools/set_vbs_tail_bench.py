#!/usr/bin/env python3
"""The end phase of a stream set with variable block size (FLAKE_AMD_SET_VBS): closing S streams whose tails differ.

For S = 16, 256 and 4096 stereo 16-bit streams (int32 samples) at levels 10 and 12, set block size 4096, the time of
closing every stream -- all tails through flake_amd_set_encode_ragged plus the read-back of every STREAMINFO -- with
the ragged leg (fhip_encode_blocks_vbs_ragged_numbered: one device batch per FLAKE_AMD_BATCH tails) and with
FLAKE_AMD_SET_RAGGED=0 (one flake_amd_set_encode call per distinct length: the behaviour before the ragged entry
covered such sets).  Both legs run in this process on the same inputs, alternating, REPS times each after a warm-up
pair, with verification off and on; the table gives the median and the min..max spread per leg and the device batches
each leg ran (flake_amd_set_device_batches).  Each repetition opens a fresh set; opening is outside the timed region.

Tails are a seeded draw from 65 .. 4095 without repetition while they last (S = 4096 repeats 65 of them), about one in
eight a multiple of 8 -- those the splitter sees.  At level 12 a multiple of 8 below 512 is made odd (+1): its eighths
would be shorter than 64 samples, where the reference has no defined result.

Also recorded: the kernel times (fhip_get_kernel_times) and the launch list of one ragged batch of the first 1024
tails.

    python tools/set_vbs_tail_bench.py [--out profiles/set_vbs_ragged_tail.txt] [--reps 7] [--sizes 16,256,4096]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flake_amd as V  # noqa: E402

CH, BITS, BS = 2, 16, 4096
LEVELS = (10, 12)


def draw_tails(S, level, seed=1):
    r = np.random.RandomState(seed)
    pool = r.permutation(np.arange(65, BS))
    t = pool[np.arange(S) % len(pool)].astype(np.int32)
    if level >= 11:
        t[(t % 8 == 0) & (t < 512)] += 1
    return t


def burst_pcm(tails, seed=2):
    """The tails back to back: every eighth of a tail a noise burst or near-silence, so that the splitter has cuts to
    find (the signal of tests/test_gpu_set_vbs.py)."""
    r = np.random.RandomState(seed)
    out = np.empty((int(tails.sum()), CH), np.int32)
    at = 0
    for n in tails:
        n = int(n)
        pat = r.randint(0, 2, 8)
        amp = np.where(np.repeat(pat, n // 8 + 1)[:n] > 0, 1 << (BITS - 3), 3)
        base = (r.uniform(-1.0, 1.0, n) * amp).astype(np.int64)
        for c in range(CH):
            out[at:at + n, c] = np.clip(base + (r.uniform(-1.0, 1.0, n) * np.maximum(amp // 16, 1)).astype(np.int64),
                                        -(1 << (BITS - 1)), (1 << (BITS - 1)) - 1)
        at += n
    return out


def close_set(S, level, pcm, tails, verify, leg):
    """One timed closing of a fresh set; returns seconds, the bytes and the device batches it took."""
    os.environ["FLAKE_AMD_SET_RAGGED"] = leg
    with V.StreamSet(S, level=level, channels=CH, bits_per_sample=BITS, flags=V.SET_VBS, block_size=BS) as st:
        st.set_verify(verify)
        sob = np.arange(S, dtype=np.int32)
        cap = 64 + pcm.size * 5 + 64 * (S + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(S, dtype=np.int32)
        t0 = time.perf_counter()
        w = st.lib.flake_amd_set_encode_ragged(st._g, pcm.ctypes.data, 4, S, tails.ctypes.data, sob.ctypes.data,
                                               out.ctypes.data, cap, sizes.ctypes.data)
        st.streaminfo(0)                                             # digests of all streams: the set is closed
        t1 = time.perf_counter()
        if w < 0:
            raise RuntimeError(st.last_error())
        return t1 - t0, bytes(out[:w]), st.device_batches()


def kernel_times(level, pcm, tails):
    """Kernel ms of one ragged batch (the first tails, at most 1024), and its launch list."""
    nb = min(len(tails), 1024)
    sz = tails[:nb]
    part = pcm[:int(sz.sum())]
    p = V.level_params(level, channels=CH, bits_per_sample=BITS, block_size=BS)
    with V.Encoder(p, max_frames=8 * nb) as enc:
        enc.set_profiling(True)
        kt = {}
        for _ in range(3):
            enc.encode_blocks_vbs_ragged_numbered(part, sz, np.zeros(nb, np.uint32))
            enc.sync()
            kt = enc.kernel_times(reset=True)
        return nb, kt, enc.last_launches()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="16,256,4096")
    a = ap.parse_args()
    batch = os.environ.get("FLAKE_AMD_BATCH", "1024")
    lines = ["# closing a stream set with variable block size: S stereo 16-bit streams (int32 samples), block %d, tails"
             " drawn from 65 .. %d, MD5 on the device, FLAKE_AMD_BATCH=%s" % (BS, BS - 1, batch),
             "# ms per closing (all tails + STREAMINFO read-back); median [min..max] of %d alternating repetitions" % a.reps,
             "# per-length = FLAKE_AMD_SET_RAGGED=0 (one call per distinct tail length), ragged = one batch per "
             "FLAKE_AMD_BATCH tails; batches = flake_amd_set_device_batches",
             "%5s %6s %7s %30s %8s %30s %8s %7s" % ("level", "S", "verify", "per-length ms", "batches", "ragged ms",
                                                    "batches", "ratio")]
    verdicts = []
    for level in LEVELS:
        for S in [int(x) for x in a.sizes.split(",")]:
            tails = draw_tails(S, level)
            pcm = np.ascontiguousarray(burst_pcm(tails))
            med = {}
            for verify in (False, True):
                t = {"0": [], "1": []}
                nbat = {}
                ref = None
                for rep in range(a.reps + 1):
                    for leg in ("0", "1"):
                        dt, data, nbat[leg] = close_set(S, level, pcm, tails, verify, leg)
                        if ref is None:
                            ref = data
                        assert data == ref, "the two legs wrote different bytes"
                        if rep:                                      # the first pair warms up
                            t[leg].append(dt * 1e3)
                fmt = lambda v: "%9.3f [%9.3f..%9.3f]" % (statistics.median(v), min(v), max(v))
                m0, m1 = statistics.median(t["0"]), statistics.median(t["1"])
                med[verify] = m1
                lines.append("%5d %6d %7s %30s %8d %30s %8d %7.2f" % (level, S, "on" if verify else "off", fmt(t["0"]),
                                                                      nbat["0"], fmt(t["1"]), nbat["1"], m0 / m1))
                print(lines[-1], flush=True)
                if S == 4096:
                    spread = max(t["0"]) - min(t["0"])
                    verdicts.append("# level %d, S = 4096, verify %s: ragged median %.3f ms %s per-length median %.3f ms "
                                    "less its own spread %.3f ms" % (level, "on" if verify else "off", m1,
                                                                     "is below" if m1 < m0 - spread else "IS NOT BELOW",
                                                                     m0, spread))
            lines.append("#   level %d, S = %d: verification adds %.3f ms to the ragged leg (%.3f -> %.3f)"
                         % (level, S, med[True] - med[False], med[False], med[True]))
        nb, kt, names = kernel_times(level, pcm, tails)
        lines.append("# level %d: kernel times of one ragged batch of %d tails, ms (launches)" % (level, nb))
        for k in ("k_prepare", "k_autocorr", "k_lpc", "k_encode", "k_assemble"):
            v = kt.get(k, (0, 0))
            lines.append("#   %-12s %8.3f (%d)" % (k, v[0], v[1]))
        lines.append("#   launches: " + ", ".join(names))
    lines += verdicts
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
