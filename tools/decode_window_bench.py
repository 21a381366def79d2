"""Windows against decoding everything: the project's headline decode batch -- 4096 stereo 16-bit frames of 4096 samples,
level 5 -- as 256 streams of 16 frames, one window of 4096 samples per stream at a random offset.
  w  flake_amd_decode_set_windows: the frames that overlap the windows are selected, uploaded and decoded, and the device
     delivers the windows alone
  p  the way without it: flake_amd_decode_set_frames over every frame (FLAKE_AMD_SET_MD5_OFF) and a slice per stream on
     the host
Then the many-files case: 4096 streams of 16 frames (the 256 streams' bytes sixteen times over), one window per stream;
w is one call, p is sixteen calls of 256 streams into one buffer, sliced call by call.  One process, the legs alternating,
the first round discarded, medians of the rest with min and max.  Then K7 alone on both legs' device batches
(fhip_set_profiling, "k_decode"): the windows' selected frames through fhip_decode_frames_windows, every frame through
fhip_decode_frames_segments.  Every w answer is compared with p's first.  Writes profiles/decode_window_bench.txt.
    python tools/decode_window_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "decode_window_bench.txt")
NF, n, ch, PER, WIN = 4096, 4096, 2, 16, 4096
S0 = NF // PER
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


pcm = np.ascontiguousarray(V.synth_pcm(NF, n, ch, 16).reshape(NF, n * ch), np.int32)
p = V.level_params(5, block_size=n, variable_block_size=0)
si = V.HostStreaminfo(min_block_size=n, max_block_size=n, sample_rate=44100, channels=ch, bits_per_sample=16)
data = []
with V.Encoder(p, max_frames=NF) as enc:
    for s in range(S0):
        part = pcm[s * PER:(s + 1) * PER]
        fb = np.zeros(PER, np.int32)
        b = V.Batch()
        b.pcm, b.nframes, b.block_size, b.frame_bytes, b.first_frame_number = part.ctypes.data, PER, n, fb.ctypes.data, 0
        cap = PER * enc.frame_stride(n) + 64
        buf = np.zeros(cap, np.uint8)
        wrote = C.c_int64(0)
        assert enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), buf.ctypes.data, cap, C.byref(wrote)) == 0
        data.append((buf[:wrote.value].copy(), fb))
hlib = V.load_host_library()
rng = np.random.default_rng(7)


def case(mult):
    """mult x 256 streams: the call's tables for both legs."""
    S = S0 * mult
    st = np.ascontiguousarray(np.tile(np.concatenate([d[0] for d in data]), mult))
    sizes = np.ascontiguousarray(np.tile(np.concatenate([d[1] for d in data]), mult))
    return dict(S=S, st=st, sizes=sizes, fow=np.full(S, PER, np.int32), sor=np.arange(S, dtype=np.int32),
                fixed=np.full(S, n, np.uint32), first=rng.integers(0, PER * n - WIN + 1, S).astype(np.uint64),
                count=np.full(S, WIN, np.int64), ws=np.zeros(S, np.int64), wst=np.zeros(S, np.int32), rs=np.zeros(S0, np.int64),
                out=np.ones((S * WIN, ch), np.int16), full=np.ones((NF * n, ch), np.int16), sliced=np.ones((S * WIN, ch), np.int16),
                bytes0=int(sum(d[0].size for d in data)))


def leg_w(c):
    g = hlib.flake_amd_decode_set_open(C.byref(si), c["S"], V.SET_MD5_OFF)
    nfd = C.c_longlong(0)
    t0 = time.perf_counter()
    got = hlib.flake_amd_decode_set_windows(g, c["S"], c["fow"].ctypes.data, c["st"].ctypes.data, c["st"].size,
                                            c["sizes"].ctypes.data, c["fixed"].ctypes.data, c["first"].ctypes.data,
                                            c["count"].ctypes.data, c["out"].ctypes.data, 2, c["S"] * WIN, c["ws"].ctypes.data,
                                            c["wst"].ctypes.data, C.byref(nfd))
    dt = (time.perf_counter() - t0) * 1e3
    assert got == c["S"] * WIN and not c["wst"].any(), hlib.flake_amd_decode_set_last_error(g)
    c["decoded"] = nfd.value
    hlib.flake_amd_decode_set_close(g)
    return dt


def leg_p(c):
    g = hlib.flake_amd_decode_set_open(C.byref(si), S0, V.SET_MD5_OFF)
    t0 = time.perf_counter()
    for k in range(c["S"] // S0):                 # 256 streams a call: every frame, then the slices
        if k:
            hlib.flake_amd_decode_set_close(g)    # (other files: their numbering starts over)
            g = hlib.flake_amd_decode_set_open(C.byref(si), S0, V.SET_MD5_OFF)
        got = hlib.flake_amd_decode_set_frames(g, S0, c["sor"].ctypes.data, c["fow"].ctypes.data, c["st"].ctypes.data, c["bytes0"],
                                               c["sizes"].ctypes.data, c["full"].ctypes.data, 2, NF * n, c["rs"].ctypes.data)
        assert got == NF * n
        for s in range(S0):
            w = k * S0 + s
            at = s * PER * n + int(c["first"][w])
            c["sliced"][w * WIN:(w + 1) * WIN] = c["full"][at:at + WIN]
    dt = (time.perf_counter() - t0) * 1e3
    hlib.flake_amd_decode_set_close(g)
    return dt


say(f"{NF} stereo 16-bit frames of {n}, level 5, as streams of {PER} frames; one window of {WIN} samples per stream at a random "
    f"offset; FLAKE_AMD_BATCH={NF}, int16 output; {rounds} timed rounds after one discarded, legs alternating; "
    f"{torch.cuda.get_device_name(0)}")
cases = {}
for mult in (1, 16):
    c = cases[mult] = case(mult)
    ms = {"w": [], "p": []}
    for r in range(rounds + 1):
        print(f"{c['S']} streams, round {r}", file=sys.stderr, flush=True)
        for k, fn in (("w", leg_w), ("p", leg_p)):
            v = fn(c)
            if r:
                ms[k].append(v)
        if r == 0:
            assert np.array_equal(c["out"], c["sliced"])
    say()
    say(f"{c['S']} streams, {c['S']} windows ({c['decoded']} of {c['S'] * PER} frames handed to the device):")
    for k, what in (("w", "flake_amd_decode_set_windows, one call"),
                    ("p", f"flake_amd_decode_set_frames over every frame ({mult} call{'s' if mult > 1 else ''}) + host slices")):
        v = ms[k]
        say(f"  {k}  {what:78s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
    say(f"  p / w per round: " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["p"], ms["w"])))

# K7 alone: the device batches of both legs through the ABI's host entries, timed as "k_decode"
say()
say('K7 alone (fhip_set_profiling, "k_decode": the header pass, the frame pass and the ends), medians of ' + str(rounds) + ":")
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_pcm_format(V.PCM_S16)
    enc.set_profiling(True)
    for mult in (1, 16):
        c = cases[mult]
        off = np.concatenate([[0], np.cumsum(c["sizes"][:NF])]).astype(np.int64)
        parts, fbs, sf, num, skip = [], [], [0], [], []
        for w in range(c["S"]):
            s = w % S0
            f0, f1 = int(c["first"][w]) // n, (int(c["first"][w]) + WIN - 1) // n
            parts.append(c["st"][off[s * PER + f0]:off[s * PER + f1 + 1]])
            fbs.append(c["sizes"][s * PER + f0:s * PER + f1 + 1])
            sf.append(sf[-1] + f1 - f0 + 1)
            num.append(f0)
            skip.append(int(c["first"][w]) - f0 * n)
        wst, wfb = np.concatenate(parts), np.concatenate(fbs)
        tw, tp = [], []
        step = 1024                               # windows a call: at most two frames each, the handle takes 4096
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            done = 0
            for a in range(0, c["S"], step):
                b = min(a + step, c["S"])
                res = enc.decode_frames_windows(np.concatenate(parts[a:b]), wfb[sf[a]:sf[b]], (b - a) * WIN,
                                                np.asarray(sf[a:b + 1]) - sf[a], skip[a:b], [WIN] * (b - a), num[a:b])
                assert res[0] == V.OK and res[2] == (b - a) * WIN
                done += 1
            kt = enc.kernel_times(reset=True)["k_decode"]
            if r:
                tw.append(kt[0])
            res = enc.decode_frames_segments(c["st"][:c["bytes0"]], c["sizes"][:NF], NF * n, np.arange(S0 + 1) * PER,
                                             np.zeros(S0, np.int64))
            assert res[0] == V.OK
            kt = enc.kernel_times(reset=True)["k_decode"]
            if r:
                tp.append(kt[0] * mult)
        say(f"  {c['S']:5d} streams: windows' frames ({len(wfb)} frames in {done} calls) {statistics.median(tw):8.3f} ms;  "
            f"every frame ({NF * mult} frames, {mult} x one call's time) {statistics.median(tp):8.3f} ms")
open(out_path, "w").write("\n".join(lines) + "\n")
