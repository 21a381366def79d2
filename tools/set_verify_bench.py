"""What verification costs a stream set, measured: 4096 blocks of 4096 stereo 16-bit samples (int16 input) spread
evenly over S streams.

    python tools/set_verify_bench.py host [S ...]   flake_amd_set_encode per 4096 blocks with verification off and on
                                                    (flake_amd_set_enable_verify; MD5 on the device), and the
                                                    single-stream pair (flake_amd_encode_frames_s16, flake_amd_set_verify
                                                    off and on) in the same process as the comparison leg: the legs
                                                    alternate call by call, the first call of each is discarded, medians
                                                    of CALLS timed calls; on-minus-off of both paths side by side.
    python tools/set_verify_bench.py one [S]        one verified flake_amd_set_encode of 4096 blocks and nothing else:
                                                    run it under `rocprofv3 --kernel-trace --stats` for the durations of
                                                    k_verify_frames and k_verify (four chunks of 1024 frames).
Defaults: S = 4096 256, CALLS = 7 (SET_VERIFY_BENCH_CALLS)."""
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
CALLS = int(os.environ.get("SET_VERIFY_BENCH_CALLS", "7"))


def buffers():
    pcm16 = np.ascontiguousarray(V.synth_pcm(NB, N, CH, 16).reshape(-1, CH).astype(np.int16))
    cap = 64 + pcm16.size * 5 + 64 * (NB + 1) * 8
    out = np.ones(cap, dtype=np.uint8)                      # touched: no page faults in the timed calls
    return pcm16, cap, out, np.zeros(NB, dtype=np.int32)


def open_set(S, verify):
    os.environ["FLAKE_AMD_BATCH"] = "1024"                  # the set's chunk
    st = V.StreamSet(S, level=5, channels=CH, bits_per_sample=16, block_size=N, order_method=V.OM_MAX)
    st.set_verify(verify)
    return st


def host(streams):
    pcm16, cap, out, sizes = buffers()
    lib = V.load_host_library()
    for S in streams:
        sob = np.ascontiguousarray(np.arange(NB) % S, dtype=np.int32)
        legs = {}
        os.environ["FLAKE_AMD_BATCH"] = "4096"              # the single-stream path's best setting (chunked, two handles)
        for name, on in (("single verify off", False), ("single verify on", True)):
            enc = V.HostEncoder(level=5, channels=CH, bits_per_sample=16, block_size=N, order_method=V.OM_MAX)
            enc.set_verify(on)
            legs[name] = (enc, lambda e=enc: lib.flake_amd_encode_frames_s16(
                C.byref(e.ctx), pcm16.ctypes.data, NB, N, 0, out.ctypes.data, cap, sizes.ctypes.data))
        for name, on in (("set verify off", False), ("set verify on", True)):
            st = open_set(S, on)
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
        for obj, _ in legs.values():
            obj.close()
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            print(f"host S={S:5d} {k:17s}: median {med[k]:7.2f} ms per {NB} blocks (min {min(v):.2f}, max {max(v):.2f}, "
                  f"{CALLS} calls)", flush=True)
        d_set, d_one = med["set verify on"] - med["set verify off"], med["single verify on"] - med["single verify off"]
        print(f"host S={S:5d} on - off: set {d_set:+.2f} ms, single stream {d_one:+.2f} ms; "
              f"set on / set off = {med['set verify on'] / med['set verify off']:.3f}; "
              f"set verify on / single verify on = {med['set verify on'] / med['single verify on']:.3f}", flush=True)


def one(streams):
    S = streams[0]
    pcm16, cap, out, sizes = buffers()
    sob = np.ascontiguousarray(np.arange(NB) % S, dtype=np.int32)
    st = open_set(S, True)
    w = V.load_host_library().flake_amd_set_encode(st._g, pcm16.ctypes.data, 2, NB, N, sob.ctypes.data,
                                                   out.ctypes.data, cap, sizes.ctypes.data)
    assert w > 0, st.last_error()
    st.close()
    print(f"one verified set call: S={S}, {NB} blocks -> {w} bytes")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "host"
    streams = [int(x) for x in sys.argv[2:]] or [4096, 256]
    {"host": host, "one": one}[mode](streams)
