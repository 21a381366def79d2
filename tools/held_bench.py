"""Windows out of held streams against the path they replace: the shapes of tools/decode_rows_bench.py -- 4096 stereo 16-bit
frames of 4096 samples, level 5, as 256 streams of 16 frames, one window of 4096 samples per stream at a random offset;
then the many-files case, 4096 streams (the 256 streams' bytes sixteen times over).  float32 rows [W][2][4096].
  r   flake_amd_decode_set_windows_rows through ctypes, its arrays prebuilt: the stream's bytes cross the link every call
  h   flake_amd_decode_set_held_windows_rows over the same windows of the same streams, held once
  pr  DecodeSet.decode_windows_rows, which builds r's arrays from a list of windows first
  ph  DecodeSet.held_windows_rows
Each leg has a set of its own, opened before the timed part (the handle's staging is grown in the discarded round); each
call allocates its rows with torch.empty, synchronises the current stream as DecodeSet.decode_windows_rows does, and
ends synchronised.  One process, the legs interleaved round by round, medians of the timed rounds with min and max, the
ratio r / h per round; the four tensors are compared for equality in the discarded round.  hold and hold_add are timed
once, on their own.  Then K7 and the gather alone (fhip_set_profiling: "k_decode", "k_gather_offsets", "k_gather_frames")
through fhip_decode_frames_windows_rows_held, 1024 windows a call.  Writes profiles/held_windows_bench.txt.
    python tools/held_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "held_windows_bench.txt")
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
    c = dict(S=S, st=np.ascontiguousarray(np.tile(np.concatenate([d[0] for d in data]), mult)),
             sizes=np.ascontiguousarray(np.tile(np.concatenate([d[1] for d in data]), mult)),
             fow=np.full(S, PER, np.int32), fixed=np.full(S, n, np.uint32),
             first=rng.integers(0, PER * n - WIN + 1, S).astype(np.uint64), count=np.full(S, WIN, np.int64),
             ws=np.zeros(S, np.int64), wst=np.zeros(S, np.int32))
    c["streams"] = [data[s % S0][0] for s in range(S)]
    # the parent's set, and the set that holds the streams: hold and hold_add timed once
    c["g_r"], c["g_pr"] = V.DecodeSet(si, 1, V.SET_MD5_OFF), V.DecodeSet(si, 1, V.SET_MD5_OFF)
    c["g_h"] = V.DecodeSet(si, 1, V.SET_MD5_OFF)
    t0 = time.perf_counter()
    c["g_h"].hold(c["st"].size)
    t1 = time.perf_counter()
    ids = []
    for a in range(0, S, S0):
        ids += c["g_h"].hold_add(c["streams"][a:a + S0], fixed_block_sizes=[n] * S0, max_block_size=n)
    c["t_hold"], c["t_add"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
    c["ids"] = np.asarray(ids, np.int32)
    assert c["g_h"].held_stats()[:2] == (c["st"].size, S * PER)
    c["wins_p"] = [(c["streams"][s], data[s % S0][1], n, int(c["first"][s]), WIN) for s in range(S)]
    c["wins_h"] = [(int(ids[s]), int(c["first"][s]), WIN) for s in range(S)]
    return c


def leg_r(c):
    g = c["g_r"]._g
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
    return dt, rows


def leg_h(c):
    g = c["g_h"]._g
    nfd = C.c_longlong(0)
    t0 = time.perf_counter()
    rows = torch.empty((c["S"], ch, WIN), dtype=torch.float32, device=dev)
    torch.cuda.current_stream(dev).synchronize()
    got = hlib.flake_amd_decode_set_held_windows_rows(g, c["S"], c["ids"].ctypes.data, c["first"].ctypes.data,
                                                      c["count"].ctypes.data, rows.data_ptr(), V.ROWS_F32, WIN,
                                                      c["ws"].ctypes.data, c["wst"].ctypes.data, C.byref(nfd))
    dt = (time.perf_counter() - t0) * 1e3
    assert got == c["S"] * WIN and not c["wst"].any() and nfd.value == c["decoded"], hlib.flake_amd_decode_set_last_error(g)
    return dt, rows


def leg_pr(c):
    t0 = time.perf_counter()
    rows = c["g_pr"].decode_windows_rows(c["wins_p"], WIN, torch.float32)[0]
    return (time.perf_counter() - t0) * 1e3, rows


def leg_ph(c):
    t0 = time.perf_counter()
    rows = c["g_h"].held_windows_rows(c["wins_h"], WIN, torch.float32)[0]
    return (time.perf_counter() - t0) * 1e3, rows


LEGS = (("r", leg_r, "flake_amd_decode_set_windows_rows, arrays prebuilt (the stream is uploaded)"),
        ("h", leg_h, "flake_amd_decode_set_held_windows_rows, arrays prebuilt (the stream is held)"),
        ("pr", leg_pr, "DecodeSet.decode_windows_rows"),
        ("ph", leg_ph, "DecodeSet.held_windows_rows"))
say(f"{NF} stereo 16-bit frames of {n}, level 5, as streams of {PER} frames; one window of {WIN} samples per stream at a random "
    f"offset, row_len {WIN}, float32 rows; FLAKE_AMD_BATCH={NF}; {rounds} timed rounds after one discarded, legs interleaved; "
    f"{torch.cuda.get_device_name(0)}")
cases = {}
for mult in (1, 16):
    c = cases[mult] = case(mult)
    ms = {k: [] for k, _, _ in LEGS}
    for r in range(rounds + 1):
        print(f"{c['S']} streams, round {r}", file=sys.stderr, flush=True)
        got = {}
        up0 = c["g_h"].held_stats()[3]
        for k, fn, _ in LEGS:
            v, got[k] = fn(c)
            if r:
                ms[k].append(v)
        if r == 0:
            assert all(torch.equal(got["r"], got[k]) for k in ("h", "pr", "ph")) and bool(got["r"].any())
            c["uploaded"] = (c["g_h"].held_stats()[3] - up0) // 2
        del got
    say()
    say(f"{c['S']} streams, {c['S']} windows ({c['decoded']} of {c['S'] * PER} frames handed to the device; the streams are "
        f"{c['st'].size / 1e6:.1f} MB, of which r stages and uploads the selected frames' bytes and h uploads "
        f"{c['uploaded'] / 1e3:.1f} KB of tables):")
    for k, _, what in LEGS:
        v = ms[k]
        say(f"  {k:2s}  {what:84s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
    say("  r / h per round:   " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["r"], ms["h"])))
    say("  pr / ph per round: " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["pr"], ms["ph"])))
    say(f"  once: hold (the store's allocation) {c['t_hold']:.2f} ms; hold_add of {c['S']} streams in {mult} calls (upload, K8, "
        f"the heads, one wait each) {c['t_add']:.2f} ms")

say()
say('K7 and the gather alone (fhip_set_profiling: "k_decode" is the header pass, the frame pass and the ends), '
    f"fhip_decode_frames_windows_rows_held over the windows' frames, 1024 windows a call, medians of {rounds}:")
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_profiling(True)
    for mult in (1, 16):
        c = cases[mult]
        store = torch.from_numpy(c["st"]).to(dev)
        off = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int64)
        srcs, fbs, sf, num, skip = [], [], [0], [], []
        for w in range(c["S"]):
            f0, f1 = int(c["first"][w]) // n, (int(c["first"][w]) + WIN - 1) // n
            srcs.append(off[w * PER + f0:w * PER + f1 + 1])
            fbs.append(c["sizes"][w * PER + f0:w * PER + f1 + 1])
            sf.append(sf[-1] + f1 - f0 + 1)
            num.append(f0)
            skip.append(int(c["first"][w]) - f0 * n)
        wsrc, wfb = np.concatenate(srcs), np.concatenate(fbs)
        rows = torch.empty((c["S"], ch, WIN), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        t7, tgo, tgf = [], [], []
        step = 1024
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            calls = 0
            for a in range(0, c["S"], step):
                b = min(a + step, c["S"])
                res = enc.decode_frames_windows_rows_held(store, c["st"].size, wsrc[sf[a]:sf[b]], wfb[sf[a]:sf[b]],
                                                          (b - a) * WIN, np.asarray(sf[a:b + 1]) - sf[a], skip[a:b],
                                                          [WIN] * (b - a), np.arange(a, b), np.zeros(b - a, np.int64), rows,
                                                          c["S"], WIN, V.ROWS_F32, seg_number=num[a:b])
                assert res[0] == V.OK and res[2] == (b - a) * WIN
                calls += 1
            kt = enc.kernel_times(reset=True)
            if r:
                t7.append(kt["k_decode"][0])
                tgo.append(kt["k_gather_offsets"][0])
                tgf.append(kt["k_gather_frames"][0])
        moved = int(wfb.sum())
        say(f"  {c['S']:5d} streams ({len(wfb)} frames, {moved / 1e6:.1f} MB, in {calls} calls): k_decode {statistics.median(t7):8.3f} ms;  "
            f"k_gather_offsets {statistics.median(tgo):6.3f} ms;  k_gather_frames {statistics.median(tgf):6.3f} ms "
            f"({2 * moved / statistics.median(tgf) / 1e6:.0f} GB/s read and written)")
        del store
for c in cases.values():
    for k in ("g_r", "g_pr", "g_h"):
        c[k].close()
open(out_path, "w").write("\n".join(lines) + "\n")
