"""Stream sets at the variable-block-size levels, measured: 4096 blocks of 4096 stereo 16-bit samples, handed over as
int32 (variable block size takes no int16), at levels 10 and 12 (block size 4096 at both), block b -> stream b % S.

    python tools/set_vbs_bench.py host [--out FILE] [S ...]
        per level: flake_amd_set_encode on a FLAKE_AMD_SET_VBS set of S streams with each stream's MD5 on the device,
        on the host (FLAKE_AMD_SET_MD5_HOST) and off, and flake_amd_encode_frames on ONE stream with its host MD5 on
        and off (FLAKE_AMD_MD5=0), all in one process: the legs alternate call by call, the first call of each is
        discarded, medians of CALLS timed calls.  The last line of a level's block is the acceptance figure: the set
        with device MD5 at the largest S against the single stream with MD5 on.  Written to FILE (default
        profiles/set_vbs_host_bench.txt) and to stdout.
    python tools/set_vbs_bench.py one [LEVEL [S]]
        one verified flake_amd_set_encode (K5 in block-table mode) and one verified flake_amd_encode_frames (K5 in
        sequence mode) of the same 4096 blocks and nothing else: run it under `rocprofv3 --kernel-trace --stats` for
        the two header kernels' durations side by side.
Defaults: S = 4096 256 16, CALLS = 7 (SET_VBS_BENCH_CALLS), FLAKE_AMD_BATCH as the environment has it (1024)."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import flake_amd  # noqa: E402

V = flake_amd
NB, N, CH, BITS = 4096, 4096, 2, 16
CALLS = int(os.environ.get("SET_VBS_BENCH_CALLS", "7"))


def buffers():
    pcm = np.ascontiguousarray(V.synth_pcm(NB, N, CH, BITS).reshape(-1, CH))
    cap = 64 + pcm.size * 5 + 64 * (NB + 1) * 8
    out = np.ones(cap, dtype=np.uint8)                      # touched: no page faults in the timed calls
    return pcm, cap, out, np.zeros(NB, dtype=np.int32)


def single(level, md5):
    old = os.environ.get("FLAKE_AMD_MD5")
    if not md5:
        os.environ["FLAKE_AMD_MD5"] = "0"
    try:
        return V.HostEncoder(level=level, channels=CH, bits_per_sample=BITS, block_size=N)
    finally:
        if not md5:
            if old is None:
                del os.environ["FLAKE_AMD_MD5"]
            else:
                os.environ["FLAKE_AMD_MD5"] = old


def host(streams, out_path):
    pcm, cap, out, sizes = buffers()
    lib = V.load_host_library()
    lines = [f"tools/set_vbs_bench.py host -- one MI355X, one process, the legs alternating call by call, first call of "
             f"each discarded, medians of {CALLS} timed calls.",
             f"{NB} blocks of {N} stereo 16-bit samples as int32 per call, block size {N} at both levels, block b -> "
             f"stream b % S, FLAKE_AMD_BATCH={os.environ.get('FLAKE_AMD_BATCH', '1024 (default)')}.",
             "  single md5 on / off   flake_amd_encode_frames on one stream, host MD5 on (default) / FLAKE_AMD_MD5=0",
             "  set md5 dev/host/off  flake_amd_set_encode on a FLAKE_AMD_SET_VBS set: K6 / FLAKE_AMD_SET_MD5_HOST / _OFF", ""]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for level in (10, 12):
        legs = {}
        for name, md5 in (("single md5 on", True), ("single md5 off", False)):
            enc = single(level, md5)
            legs[name] = (enc, None, lambda e=enc: lib.flake_amd_encode_frames(
                C.byref(e.ctx), pcm.ctypes.data, NB, N, 0, out.ctypes.data, cap, sizes.ctypes.data))
        for S in streams:
            sob = np.ascontiguousarray(np.arange(NB) % S, dtype=np.int32)
            for name, flags in (("md5 dev", 0), ("md5 host", V.SET_MD5_HOST), ("md5 off", V.SET_MD5_OFF)):
                st = V.StreamSet(S, level=level, channels=CH, bits_per_sample=BITS, flags=flags | V.SET_VBS,
                                 block_size=N)
                legs[f"set S={S} {name}"] = (st, sob, lambda g=st, o=sob: lib.flake_amd_set_encode(
                    g._g, pcm.ctypes.data, 4, NB, N, o.ctypes.data, out.ctypes.data, cap, sizes.ctypes.data))
        ms = {k: [] for k in legs}
        for call in range(CALLS + 1):
            for name, (_, _, fn) in legs.items():
                t0 = time.perf_counter()
                w = fn()
                dt = (time.perf_counter() - t0) * 1e3
                assert w > 0, name
                if call:
                    ms[name].append(dt)
        for obj, _, _ in legs.values():
            obj.close()
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, v in ms.items():
            say(f"level {level:2d} {k:22s}: median {med[k]:8.2f} ms per {NB} blocks (min {min(v):.2f}, max {max(v):.2f})")
        top = max(streams)
        a, b = med[f"set S={top} md5 dev"], med["single md5 on"]
        say(f"level {level:2d} acceptance: set S={top} md5 dev / single md5 on = {a:.2f} / {b:.2f} = {a / b:.3f} "
            f"(required below 0.5: {'met' if a < 0.5 * b else 'MISSED'}); single md5 on / off = "
            f"{b / med['single md5 off']:.2f}; set md5 dev / set md5 off = {a / med[f'set S={top} md5 off']:.2f}")
        say("")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines))


def one(level, S):
    pcm, cap, out, sizes = buffers()
    lib = V.load_host_library()
    sob = np.ascontiguousarray(np.arange(NB) % S, dtype=np.int32)
    with V.StreamSet(S, level=level, channels=CH, bits_per_sample=BITS, flags=V.SET_VBS, block_size=N) as st:
        st.set_verify(True)
        w = lib.flake_amd_set_encode(st._g, pcm.ctypes.data, 4, NB, N, sob.ctypes.data, out.ctypes.data, cap,
                                     sizes.ctypes.data)
        assert w > 0, st.last_error()
    with V.HostEncoder(level=level, channels=CH, bits_per_sample=BITS, block_size=N) as enc:
        enc.set_verify(True)
        w1 = lib.flake_amd_encode_frames(C.byref(enc.ctx), pcm.ctypes.data, NB, N, 0, out.ctypes.data, cap,
                                         sizes.ctypes.data)
        assert w1 > 0
    print(f"one verified call each: level {level}, set of {S} streams -> {w} bytes, single stream -> {w1} bytes")


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = args.pop(0) if args else "host"
    if mode == "one":
        one(int(args[0]) if args else 10, int(args[1]) if len(args) > 1 else 4096)
    else:
        out_path = os.path.join(ROOT, "profiles", "set_vbs_host_bench.txt")
        if args and args[0] == "--out":
            out_path = args[1]
            args = args[2:]
        host([int(x) for x in args] or [4096, 256, 16], out_path)
