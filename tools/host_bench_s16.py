"""int16 against int32 input through the host C layer: the same 4096 x 4096 stereo 16-bit frames through
flake_amd_encode_frames (the samples widened to int32, as every caller had to) and
flake_amd_encode_frames_s16, alternating in one process, for both batch settings and with the stream MD5
on and off.  The first call of each width is discarded (one-time costs), the rest are timed; the int32
calls of the same run are the yardstick.
    python tools/host_bench_s16.py [frames] [timed calls per width]"""
import ctypes as C, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, flake_amd

nfr = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n, ch = 4096, 2
pcm32 = np.ascontiguousarray(flake_amd.synth_pcm(nfr, n, ch, 16).reshape(-1, ch))
pcm16 = np.ascontiguousarray(pcm32.astype(np.int16))
cap = 64 + pcm32.size * 5 + 64 * (nfr + 1) * 8
out = np.ones(cap, dtype=np.uint8)                      # touched: no page faults in the timed calls
sizes = np.zeros(nfr, dtype=np.int32)
for md5 in ("1", "0"):
    for batch in (1024, 4096):
        os.environ["FLAKE_AMD_BATCH"] = str(batch)
        os.environ["FLAKE_AMD_MD5"] = md5
        enc = flake_amd.HostEncoder(level=5, channels=ch, bits_per_sample=16, sample_rate=44100, block_size=n,
                                    order_method=flake_amd.OM_MAX)
        ms = {"s32": [], "s16": []}
        for call in range(calls + 1):
            for name, fn, buf in (("s32", enc.lib.flake_amd_encode_frames, pcm32),
                                  ("s16", enc.lib.flake_amd_encode_frames_s16, pcm16)):
                t0 = time.perf_counter()
                w = fn(C.byref(enc.ctx), buf.ctypes.data, nfr, n, 0, out.ctypes.data, cap, sizes.ctypes.data)
                dt = (time.perf_counter() - t0) * 1e3
                assert w > 0, enc.lib.flake_amd_last_error(C.byref(enc.ctx))
                if call:
                    ms[name].append(dt)
        enc.close()
        m32, m16 = statistics.median(ms["s32"]), statistics.median(ms["s16"])
        print(f"md5 {'on' if md5 == '1' else 'off'} batch {batch}: {nfr} frames; int32 median {m32:.2f} ms "
              f"(min {min(ms['s32']):.2f}, max {max(ms['s32']):.2f}); int16 median {m16:.2f} ms "
              f"(min {min(ms['s16']):.2f}, max {max(ms['s16']):.2f}); int16 - int32 = {m16 - m32:+.2f} ms; "
              f"{(pcm32.nbytes - pcm16.nbytes) / 1e6:.0f} MB fewer uploaded", flush=True)
