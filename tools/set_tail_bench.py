#!/usr/bin/env python3
"""The end phase of a stream set: from the last full batch to the closed set.

For S = 16, 256 and 4096 stereo 16-bit streams at level 5 with pairwise distinct tail lengths (MD5 on the device,
verification off and on), the time of closing every stream -- all tails through flake_amd_set_encode_ragged plus the
read-back of every STREAMINFO -- with FLAKE_AMD_SET_RAGGED=1 (one ragged call) and =0 (one uniform call per distinct
length, the behaviour before the ragged entry existed).  Both legs run in this process on the same inputs,
interleaved, REPS times each after a warm-up pair; the table gives the median and the min..max spread per leg.
Each repetition opens a fresh set (a closed stream cannot be closed twice); opening is outside the timed region.

Also recorded: the kernel times (fhip_get_kernel_times) of the ragged K1 and K3 instances over the S = 4096 tails,
beside the uniform generic instances (FHIP_K3_GENERIC=1 is not needed: an odd length has no tuned geometry) over the
same number of frames at the mean tail length.

    python tools/set_tail_bench.py [--out profiles/set_ragged_tail.txt] [--reps 7] [--sizes 16,256,4096]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flake_amd as V  # noqa: E402

LEVEL, CH, BITS = 5, 2, 16


def distinct_tails(S, bs, seed=1):
    # distinct lengths in 1 .. bs - 1, shuffled (with S > bs - 1 streams the lengths wrap: S = bs repeats one)
    r = np.random.RandomState(seed)
    return (r.permutation(np.arange(S) % (bs - 1)) + 1).astype(np.int32)


def close_set(S, pcm, tails, verify, leg):
    """One timed closing of a fresh set; returns seconds."""
    os.environ["FLAKE_AMD_SET_RAGGED"] = leg
    os.environ["FLAKE_AMD_BATCH"] = "4096"
    with V.StreamSet(S, level=LEVEL, channels=CH, bits_per_sample=BITS) as st:
        st.set_verify(verify)
        sob = np.arange(S, dtype=np.int32)
        cap = 64 + pcm.size * 5 + 64 * (S + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(S, dtype=np.int32)
        t0 = time.perf_counter()
        w = st.lib.flake_amd_set_encode_ragged(st._g, pcm.ctypes.data, 2, S, tails.ctypes.data, sob.ctypes.data,
                                               out.ctypes.data, cap, sizes.ctypes.data)
        st.streaminfo(0)                                             # digests of all streams: the set is closed
        t1 = time.perf_counter()
        if w < 0:
            raise RuntimeError(st.last_error())
        return t1 - t0, bytes(out[:w])


def kernel_times(S, bs, tails, pcm):
    """K1 / K3 ms over the S tails: the ragged instances, and the uniform generic ones at the mean tail length."""
    p = V.level_params(LEVEL, channels=CH, bits_per_sample=BITS)
    res = {}
    with V.Encoder(p, max_frames=S) as enc:
        enc.set_pcm_format(V.PCM_S16)
        enc.set_profiling(True)
        fb = np.zeros(S, np.int32)
        total = C.c_int64(0)
        b = V.Batch(pcm=pcm.ctypes.data, nframes=S, block_size=int(tails.max()), frame_bytes=fb.ctypes.data)
        for _ in range(3):
            rc = enc.lib.fhip_frames_packed_begin_ragged(enc._h, C.byref(b), tails.ctypes.data, C.byref(total))
            assert rc == V.OK, rc
            enc.sync()
            res["ragged"] = enc.kernel_times(reset=True)
        res["ragged_launches"] = enc.last_launches()
        mean = int(tails.mean()) | 1                                 # odd: the generic K3, no tuned geometry
        upcm = np.ascontiguousarray(pcm[:S * mean])
        b = V.Batch(pcm=upcm.ctypes.data, nframes=S, block_size=mean, frame_bytes=fb.ctypes.data)
        for _ in range(3):
            rc = enc.lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total))
            assert rc == V.OK, rc
            enc.sync()
            res["uniform"] = enc.kernel_times(reset=True)
        res["uniform_launches"] = enc.last_launches()
        res["mean"] = mean
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="16,256,4096")
    a = ap.parse_args()
    bs = V.level_params(LEVEL).block_size
    lines = ["# closing a stream set: S stereo 16-bit streams, level 5, block %d, distinct tails, MD5 on the device" % bs,
             "# ms per closing (all tails + STREAMINFO read-back); median [min..max] of %d interleaved repetitions" % a.reps,
             "# per-length = FLAKE_AMD_SET_RAGGED=0 (one uniform call per tail), ragged = one call",
             "%6s %7s %28s %28s %8s" % ("S", "verify", "per-length ms", "ragged ms", "ratio")]
    for S in [int(x) for x in a.sizes.split(",")]:
        tails = distinct_tails(S, bs)
        pcm = np.ascontiguousarray(V.synth_pcm((int(tails.sum()) + bs - 1) // bs, bs, CH, BITS).reshape(-1, CH)
                                   [:int(tails.sum())].astype(np.int16))
        for verify in (False, True):
            t = {"0": [], "1": []}
            ref = None
            for rep in range(a.reps + 1):
                for leg in ("0", "1"):
                    dt, data = close_set(S, pcm, tails, verify, leg)
                    if ref is None:
                        ref = data
                    assert data == ref, "the two legs wrote different bytes"
                    if rep:                                          # the first pair warms up
                        t[leg].append(dt * 1e3)
            fmt = lambda v: "%9.3f [%9.3f..%9.3f]" % (statistics.median(v), min(v), max(v))
            lines.append("%6d %7s %28s %28s %8.2f" % (S, "on" if verify else "off", fmt(t["0"]), fmt(t["1"]),
                                                      statistics.median(t["0"]) / statistics.median(t["1"])))
            print(lines[-1], flush=True)
        if S == 4096:
            kt = kernel_times(S, bs, tails, pcm)
            lines.append("# kernel times over %d frames, ms (launches): ragged tails (mean length %d) | uniform generic "
                         "instances at n = %d" % (S, int(tails.mean()), kt["mean"]))
            for k in ("k_prepare", "k_autocorr", "k_lpc", "k_encode", "k_assemble"):
                r, u = kt["ragged"].get(k, (0, 0)), kt["uniform"].get(k, (0, 0))
                lines.append("#   %-12s ragged %8.3f (%d)   uniform %8.3f (%d)" % (k, r[0], r[1], u[0], u[1]))
            lines.append("#   ragged launches:  " + ", ".join(kt["ragged_launches"]))
            lines.append("#   uniform launches: " + ", ".join(kt["uniform_launches"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
