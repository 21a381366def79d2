"""Cost of K5 (the on-device verifier), one JSON line per case.

    python tools/verify_bench.py [--reps R]

kernel cases: the stream is encoded once, then fhip_verify_frames_dev runs R times on the device-resident
stream and PCM with profiling on (hipEvents around the three launches: k_verify in the kernel table);
configs[1] = 4096 stereo 16-bit frames of 4096, LPC-8 (level 5, order method MAX); level 8; configs[3] =
8 channels, 24 bits, LPC-12; level 12 variable block size with 1024 blocks (fhip_encode_blocks_vbs_dev
with verification on: k_verify per batch).
host cases: flake_amd_encode_frames on 4096 frames (tools/host_bench.py's setup), verification off and on.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import flake_amd  # noqa: E402

P = flake_amd.level_params


def packed(enc, pcm, n):
    nf = pcm.shape[0]
    fb = np.zeros(nf, np.int32)
    b = flake_amd.Batch()
    b.pcm, b.nframes, b.block_size, b.frame_bytes = pcm.ctypes.data, nf, n, fb.ctypes.data
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = C.c_int64(0)
    rc = enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), out.ctypes.data, cap, C.byref(wrote))
    assert rc == 0, enc.lib.fhip_last_error(enc._h)
    return out[:wrote.value], fb


def kernel_case(name, p, nframes, reps):
    n = p.block_size
    pcm = flake_amd.synth_pcm(nframes, n, p.channels, p.bits_per_sample)
    with flake_amd.Encoder(p, max_frames=nframes) as enc:
        s, fb = packed(enc, pcm, n)
        dev = torch.device("cuda")
        ds, dfb = torch.from_numpy(s.copy()).to(dev), torch.from_numpy(fb).to(dev)
        dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
        dsum = torch.zeros(4, dtype=torch.int64, device=dev)
        args = (ds, len(s), dfb, nframes, dp, nframes * n, 0, dsum)
        enc.verify_frames_dev(*args)           # first launch: code objects, workspace
        enc.sync()
        enc.set_profiling(True)
        enc.kernel_times(reset=True)
        t0 = time.perf_counter()
        for _ in range(reps):
            enc.verify_frames_dev(*args)
        enc.sync()
        wall = (time.perf_counter() - t0) / reps
        kt = enc.kernel_times(reset=True)
        ok = int(dsum[1]) == 0
    ms, cnt = kt["k_verify"]
    return {"case": name, "frames": nframes, "block": n, "channels": p.channels, "bps": p.bits_per_sample,
            "stream_bytes": int(len(s)), "k_verify_ms": round(ms / cnt, 4), "wall_ms": round(wall * 1e3, 4),
            "all_ok": ok}


def vbs_case(reps):
    p = P(12)
    n, nb = p.block_size, 1024
    pcm = flake_amd.synth_pcm(nb, n, 2, 16)
    with flake_amd.Encoder(p, max_frames=8 * nb) as enc:
        dev = torch.device("cuda")
        dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
        cap = 8 * nb * enc.frame_stride(n)
        dpk = torch.zeros(cap, dtype=torch.uint8, device=dev)
        dt = torch.zeros(4, dtype=torch.int64, device=dev)
        res = {}
        for on in (False, True):
            enc.set_verify(on)
            enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt)
            enc.sync()
            enc.set_profiling(True)
            enc.kernel_times(reset=True)
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt)
            enc.sync()
            res[on] = ((time.perf_counter() - t0) / reps, enc.kernel_times(reset=True))
            enc.set_profiling(False)
        flags = int(dt[3])
    ms, cnt = res[True][1]["k_verify"]
    return {"case": "level12_vbs_1024_blocks", "blocks": nb, "block": n, "frames": int(dt[0]),
            "k_verify_ms": round(ms / cnt, 4), "step_ms_off": round(res[False][0] * 1e3, 3),
            "step_ms_on": round(res[True][0] * 1e3, 3), "verify_flag": bool(flags & 4)}


def host_case(calls=4):
    nfr, n = 4096, 4096
    pcm = flake_amd.synth_pcm(nfr, n, 2, 16).reshape(-1, 2)
    cap = 64 + pcm.size * 5 + 64 * (nfr + 1) * 8
    out = np.ones(cap, dtype=np.uint8)
    sizes = np.zeros(nfr, dtype=np.int32)
    res = {}
    for on in (False, True):
        enc = flake_amd.HostEncoder(level=5, block_size=n, order_method=flake_amd.OM_MAX)
        enc.set_verify(on)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            w = enc.lib.flake_amd_encode_frames(C.byref(enc.ctx), pcm.ctypes.data, nfr, n, 0, out.ctypes.data, cap,
                                                sizes.ctypes.data)
            ts.append(time.perf_counter() - t0)
            assert w > 0, enc.lib.flake_amd_last_error(C.byref(enc.ctx))
        enc.close()
        res[on] = min(ts[1:]) * 1e3
    return {"case": "host_4096x4096_level5_max", "ms_off": round(res[False], 2), "ms_on": round(res[True], 2),
            "overhead_pct": round(100 * (res[True] / res[False] - 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    cases = [
        ("configs1_lpc8_max", P(5, order_method=flake_amd.OM_MAX), 4096),
        ("level8", P(8), 4096),
        ("configs3_8ch24_lpc12", P(5, channels=8, bits_per_sample=24, sample_rate=192000,
                                   order_method=flake_amd.OM_MAX, max_prediction_order=12), 1024),
    ]
    for name, p, nf in cases:
        if not a.only or a.only == name:
            print(json.dumps(kernel_case(name, p, nf, a.reps)), flush=True)
    if not a.only or a.only == "vbs":
        print(json.dumps(vbs_case(max(3, a.reps // 4))), flush=True)
    if not a.only or a.only == "host":
        print(json.dumps(host_case()), flush=True)


if __name__ == "__main__":
    main()
