"""Windows as rows on the device against the composition a caller had before: the shapes of tools/decode_window_bench.py --
4096 stereo 16-bit frames of 4096 samples, level 5, as 256 streams of 16 frames, one window of 4096 samples per stream at
a random offset; then the many-files case, 4096 streams (the 256 streams' bytes sixteen times over).  Every window asks
for exactly row_len samples, so there is nothing to pad.
  r  flake_amd_decode_set_windows_rows into a float32 tensor [W][2][4096] from torch.empty (the current stream
     synchronised first, as DecodeSet.decode_windows_rows does)
  c  flake_amd_decode_set_windows into host int16, torch.from_numpy(...).to(device), view and permute to [W][C][T],
     convert to float32 and scale, contiguous
Both legs end synchronised and their tensors are compared for equality in the discarded round.  One process, the legs
alternating, medians of the timed rounds with min and max.  Then K7 and K10 alone on the windows' frames
(fhip_set_profiling: "k_decode", "k_window_rows") through fhip_decode_frames_windows_rows, 1024 windows a call.
Writes profiles/decode_rows_bench.txt.
    python tools/decode_rows_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "decode_rows_bench.txt")
NF, n, ch, PER, WIN = 4096, 4096, 2, 16, 4096
S0 = NF // PER
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


hlib = V.load_host_library()
dev = torch.device("cuda", 0)
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
rng = np.random.default_rng(7)


def case(mult):
    S = S0 * mult
    return dict(S=S, st=np.ascontiguousarray(np.tile(np.concatenate([d[0] for d in data]), mult)),
                sizes=np.ascontiguousarray(np.tile(np.concatenate([d[1] for d in data]), mult)),
                fow=np.full(S, PER, np.int32), fixed=np.full(S, n, np.uint32),
                first=rng.integers(0, PER * n - WIN + 1, S).astype(np.uint64), count=np.full(S, WIN, np.int64),
                ws=np.zeros(S, np.int64), wst=np.zeros(S, np.int32), host=np.ones((S * WIN, ch), np.int16))


def leg_r(c):
    g = hlib.flake_amd_decode_set_open(C.byref(si), c["S"], V.SET_MD5_OFF)
    nfd = C.c_longlong(0)
    t0 = time.perf_counter()
    rows = torch.empty((c["S"], ch, WIN), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    got = hlib.flake_amd_decode_set_windows_rows(g, c["S"], c["fow"].ctypes.data, c["st"].ctypes.data, c["st"].size,
                                                 c["sizes"].ctypes.data, c["fixed"].ctypes.data, c["first"].ctypes.data,
                                                 c["count"].ctypes.data, rows.data_ptr(), V.ROWS_F32, WIN, c["ws"].ctypes.data,
                                                 c["wst"].ctypes.data, C.byref(nfd))
    dt = (time.perf_counter() - t0) * 1e3
    assert got == c["S"] * WIN and not c["wst"].any(), hlib.flake_amd_decode_set_last_error(g)
    c["decoded"] = nfd.value
    hlib.flake_amd_decode_set_close(g)
    return dt, rows


def leg_c(c):
    g = hlib.flake_amd_decode_set_open(C.byref(si), c["S"], V.SET_MD5_OFF)
    nfd = C.c_longlong(0)
    t0 = time.perf_counter()
    got = hlib.flake_amd_decode_set_windows(g, c["S"], c["fow"].ctypes.data, c["st"].ctypes.data, c["st"].size,
                                            c["sizes"].ctypes.data, c["fixed"].ctypes.data, c["first"].ctypes.data,
                                            c["count"].ctypes.data, c["host"].ctypes.data, 2, c["S"] * WIN, c["ws"].ctypes.data,
                                            c["wst"].ctypes.data, C.byref(nfd))
    t1 = time.perf_counter()
    rows = (torch.from_numpy(c["host"]).to(dev).view(c["S"], WIN, ch).permute(0, 2, 1).to(torch.float32) * 2.0 ** -15).contiguous()
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    assert got == c["S"] * WIN and not c["wst"].any(), hlib.flake_amd_decode_set_last_error(g)
    hlib.flake_amd_decode_set_close(g)
    c["tail"].append((t2 - t1) * 1e3)
    return (t2 - t0) * 1e3, rows


say(f"{NF} stereo 16-bit frames of {n}, level 5, as streams of {PER} frames; one window of {WIN} samples per stream at a random "
    f"offset, row_len {WIN}, float32 rows; FLAKE_AMD_BATCH={NF}; {rounds} timed rounds after one discarded, legs alternating; "
    f"{torch.cuda.get_device_name(0)}")
cases = {}
for mult in (1, 16):
    c = cases[mult] = case(mult)
    ms = {"r": [], "c": []}
    for r in range(rounds + 1):
        print(f"{c['S']} streams, round {r}", file=sys.stderr, flush=True)
        c["tail"] = c.get("tail", []) if r else []
        got = {}
        for k, fn in (("r", leg_r), ("c", leg_c)):
            v, got[k] = fn(c)
            if r:
                ms[k].append(v)
        if r == 0:
            assert torch.equal(got["r"], got["c"])
            c["tail"] = []
        del got
    say()
    say(f"{c['S']} streams, {c['S']} windows ({c['decoded']} of {c['S'] * PER} frames handed to the device):")
    for k, what in (("r", "flake_amd_decode_set_windows_rows -> float32 [W][C][T] on the device"),
                    ("c", "flake_amd_decode_set_windows -> host int16, upload, permute, convert, scale")):
        v = ms[k]
        say(f"  {k}  {what:78s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
    say(f"     of c, behind the decode call (upload and the torch kernels): {statistics.median(c['tail']):.2f} ms")
    say(f"  c / r per round: " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["c"], ms["r"])))

say()
say('K7 and K10 alone (fhip_set_profiling: "k_decode" is the header pass, the frame pass and the ends; "k_window_rows"), '
    f"fhip_decode_frames_windows_rows over the windows' frames, 1024 windows a call, medians of {rounds}:")
with V.Encoder(p, max_frames=NF) as enc:
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
        wfb = np.concatenate(fbs)
        rows = torch.empty((c["S"], ch, WIN), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        t7, t10 = [], []
        step = 1024
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            calls = 0
            for a in range(0, c["S"], step):
                b = min(a + step, c["S"])
                res = enc.decode_frames_windows_rows(np.concatenate(parts[a:b]), wfb[sf[a]:sf[b]], (b - a) * WIN,
                                                     np.asarray(sf[a:b + 1]) - sf[a], skip[a:b], [WIN] * (b - a),
                                                     np.arange(a, b), np.zeros(b - a, np.int64), rows, c["S"], WIN, V.ROWS_F32,
                                                     seg_number=num[a:b])
                assert res[0] == V.OK and res[2] == (b - a) * WIN
                calls += 1
            kt = enc.kernel_times(reset=True)
            if r:
                t7.append(kt["k_decode"][0])
                t10.append(kt["k_window_rows"][0])
        say(f"  {c['S']:5d} streams ({len(wfb)} frames in {calls} calls): k_decode {statistics.median(t7):8.3f} ms;  "
            f"k_window_rows {statistics.median(t10):7.3f} ms "
            f"({c['S'] * WIN * ch * 8 / statistics.median(t10) / 1e6:.0f} GB/s of int32 read and float32 written)")
open(out_path, "w").write("\n".join(lines) + "\n")
