"""K6 and the stream set, measured: 4096 blocks of 4096 stereo 16-bit samples spread evenly over S streams.

    python tools/md5_bench.py kernel [S ...]     k_md5_streams alone on device-resident PCM, from int32 and from int16:
                                                 milliseconds between events on the launch stream, median of the timed
                                                 launches, and the message bytes hashed per second.  Run it under
                                                 `rocprofv3 --kernel-trace --stats` for the profiler's own durations
                                                 (dispatches in this order: per S, int32 then int16, 1 + CALLS each).
    python tools/md5_bench.py host [S ...]       flake_amd_set_encode per 4096 blocks with the MD5 on the device, on the
                                                 host and off, against the single-stream path (flake_amd_encode_frames_s16,
                                                 MD5 on and off) in the same process: the legs alternate call by call, the
                                                 first call of each is discarded, medians of CALLS timed calls.
Defaults: S = 16 256 4096, CALLS = 7 (MD5_BENCH_CALLS)."""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import flake_amd  # noqa: E402

V = flake_amd
NB, N, CH = 4096, 4096, 2
CALLS = int(os.environ.get("MD5_BENCH_CALLS", "7"))


def kernel(streams):
    import torch
    dev = torch.device("cuda", 0)
    p = V.level_params(5, order_method=V.OM_MAX)
    pcm32 = np.ascontiguousarray(V.synth_pcm(NB, N, CH, 16).reshape(-1, CH))
    msg_bytes = NB * N * CH * 2
    side = torch.cuda.Stream()              # (not the null stream: fhip_set_stream(NULL) means the handle's own)
    with V.Encoder(p, max_frames=4) as enc, torch.cuda.stream(side):
        enc.set_stream(side.cuda_stream)
        for S in streams:
            # block b belongs to stream b % S: the round-robin batch a multi-file caller hands over
            sob = np.arange(NB) % S
            seg_block = torch.from_numpy(np.argsort(sob, kind="stable").astype(np.int32)).to(dev)
            seg_first = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(sob, minlength=S))]).astype(np.int32)).to(dev)
            states = torch.zeros(S * V.MD5_STATE_BYTES, dtype=torch.uint8, device=dev)
            for fmt, name, host in ((V.PCM_S32, "int32", pcm32), (V.PCM_S16, "int16", pcm32.astype(np.int16))):
                enc.set_pcm_format(fmt)
                pcm = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
                torch.cuda.synchronize()
                enc.md5_init_dev(states, S)
                ms = []
                for call in range(CALLS + 1):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    enc.md5_update_dev(states, S, pcm, N, seg_first, seg_block)
                    b.record()
                    b.synchronize()
                    if call:
                        ms.append(a.elapsed_time(b))
                path = enc.last_launches()[-1]
                m = statistics.median(ms)
                print(f"kernel S={S:5d} {name}: median {m:8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) of {CALLS} "
                      f"launches, {msg_bytes / m / 1e6:8.2f} GB/s hashed, {NB // S} blocks per stream; {path}", flush=True)
                del pcm
    print("(event times include k_md5_scan, a single-workgroup launch of a few microseconds)")


def host(streams):
    pcm16 = np.ascontiguousarray(V.synth_pcm(NB, N, CH, 16).reshape(-1, CH).astype(np.int16))
    cap = 64 + pcm16.size * 5 + 64 * (NB + 1) * 8
    out = np.ones(cap, dtype=np.uint8)                      # touched: no page faults in the timed calls
    sizes = np.zeros(NB, dtype=np.int32)
    os.environ["FLAKE_AMD_BATCH"] = "4096"                  # the single-stream path's best setting (chunked, two handles)
    lib = V.load_host_library()
    for S in streams:
        sob = np.ascontiguousarray(np.arange(NB) % S, dtype=np.int32)
        legs = {}
        for name, md5 in (("single md5 on", "1"), ("single md5 off", "0")):
            os.environ["FLAKE_AMD_MD5"] = md5
            enc = V.HostEncoder(level=5, channels=CH, bits_per_sample=16, block_size=N, order_method=V.OM_MAX)
            legs[name] = (enc, lambda e=enc: lib.flake_amd_encode_frames_s16(
                C.byref(e.ctx), pcm16.ctypes.data, NB, N, 0, out.ctypes.data, cap, sizes.ctypes.data))
        os.environ.pop("FLAKE_AMD_MD5")
        os.environ["FLAKE_AMD_BATCH"] = "1024"              # the set's chunk
        for name, flags in (("set md5 device", 0), ("set md5 host", V.SET_MD5_HOST), ("set md5 off", V.SET_MD5_OFF)):
            st = V.StreamSet(S, level=5, channels=CH, bits_per_sample=16, flags=flags, block_size=N,
                             order_method=V.OM_MAX)
            legs[name] = (st, lambda g=st: lib.flake_amd_set_encode(
                g._g, pcm16.ctypes.data, 2, NB, N, sob.ctypes.data, out.ctypes.data, cap, sizes.ctypes.data))
        os.environ["FLAKE_AMD_BATCH"] = "4096"
        ms = {k: [] for k in legs}
        for call in range(CALLS + 1):
            for name, (_, fn) in legs.items():
                t0 = time.perf_counter()
                w = fn()
                dt = (time.perf_counter() - t0) * 1e3
                assert w > 0, name
                if call:
                    ms[name].append(dt)
        t0 = time.perf_counter()
        legs["set md5 device"][0].streaminfo(0)             # all digests: one finalisation, one read-back
        t_fin = (time.perf_counter() - t0) * 1e3
        for obj, _ in legs.values():
            obj.close()
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            print(f"host S={S:5d} {k:15s}: median {med[k]:7.2f} ms per {NB} blocks (min {min(v):.2f}, max {max(v):.2f}, "
                  f"{CALLS} calls)", flush=True)
        print(f"host S={S:5d} ratios: set md5 device / single md5 on = {med['set md5 device'] / med['single md5 on']:.3f}; "
              f"set md5 off / single md5 off = {med['set md5 off'] / med['single md5 off']:.3f}; "
              f"set md5 device - set md5 off = {med['set md5 device'] - med['set md5 off']:+.2f} ms; "
              f"digests of all {S} streams fetched in {t_fin:.2f} ms", flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    streams = [int(x) for x in sys.argv[2:]] or [16, 256, 4096]
    {"kernel": kernel, "host": host}[mode](streams)
