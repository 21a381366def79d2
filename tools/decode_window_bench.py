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
Last, what a SEEKTABLE buys one file: the 4096 frames as ONE file, written by flake_amd_cli with --seekpoints 441000 and
without, one window of 4096 samples out of each by the steps of `flake_amd_cli --decode --skip --until`:
  t  the piece between two seek points indexed (flake_amd_index_frames), then flake_amd_decode_set_windows over it
  n  no table: the whole file indexed on the device (flake_amd_decode_set_index, K8), then the same entry over all of it
    python tools/decode_window_bench.py [timed rounds] [output file] [seek]
With `seek` as the third argument only that last leg runs, and its section replaces the one in the output file."""
import ctypes as C, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "decode_window_bench.txt")
SEEK_ONLY = len(sys.argv) > 3 and sys.argv[3] == "seek"
SEEK_MARK = "One file of "
NF, n, ch, PER, WIN = 4096, 4096, 2, 16, 4096
S0 = NF // PER
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


hlib = V.load_host_library()


def seek_leg():
    """One window out of one long file, with a SEEKTABLE and without."""
    SPACING, SKIP = 441000, NF * n // 2 + 1234
    cli = os.path.join(V.LIB_DIR, "flake_amd_cli")
    files = {}
    with tempfile.TemporaryDirectory() as d:
        for k, extra in (("t", ["--seekpoints", str(SPACING)]), ("n", [])):
            path = os.path.join(d, k + ".flac")
            subprocess.run([cli, "--synth", str(NF), "-b", str(n), *extra, path], check=True, capture_output=True, timeout=600)
            raw = np.fromfile(path, np.uint8)
            at, table, last = 4, None, 0
            while not last:                       # the metadata blocks: STREAMINFO, the SEEKTABLE where there is one
                last, kind, size = raw[at] >> 7, raw[at] & 0x7F, int.from_bytes(raw[at + 1:at + 4].tobytes(), "big")
                if kind == 3:
                    table = raw[at + 4:at + 4 + size].tobytes()
                at += 4 + size
            files[k] = dict(si=V.read_streaminfo(raw[8:42].tobytes())[0], frames=np.ascontiguousarray(raw[at:]), table=table)
    assert files["t"]["table"] and not files["n"]["table"] and np.array_equal(files["t"]["frames"], files["n"]["frames"])
    fsi = files["n"]["si"]
    g = hlib.flake_amd_decode_set_open(C.byref(fsi), 1, V.SET_MD5_OFF)
    assert g, hlib.flake_amd_decode_set_last_error(None)
    out = {k: np.ones((WIN, ch), np.int16) for k in files}
    indexed, cap_all = {}, files["n"]["frames"].size // 8 + 2
    all_sizes = np.zeros(cap_all, np.int32)

    def window(k, piece, sizes):
        fow, fixed = np.asarray([len(sizes)], np.int32), np.asarray([n], np.uint32)
        first, count = np.asarray([SKIP], np.uint64), np.asarray([WIN], np.int64)
        ws, wst, nfd = np.zeros(1, np.int64), np.zeros(1, np.int32), C.c_longlong(0)
        got = hlib.flake_amd_decode_set_windows(g, 1, fow.ctypes.data, piece.ctypes.data, piece.size, sizes.ctypes.data,
                                                fixed.ctypes.data, first.ctypes.data, count.ctypes.data, out[k].ctypes.data, 2,
                                                WIN, ws.ctypes.data, wst.ctypes.data, C.byref(nfd))
        assert got == WIN and not wst.any(), hlib.flake_amd_decode_set_last_error(g)
        indexed[k] = (len(sizes), nfd.value)

    def leg_t():
        f = files["t"]
        t0 = time.perf_counter()
        pts, _ = V.read_seektable(f["table"])
        a, b = V.seek_lookup(pts, SKIP), V.seek_lookup(pts, SKIP + WIN - 1) + 1
        lo = int(pts[a]["offset"]) if a >= 0 else 0
        hi = int(pts[b]["offset"]) if b < len(pts) else f["frames"].size
        piece = f["frames"][lo:hi]
        sizes, used = V.index_frames(f["si"], piece)
        assert used == piece.size
        window("t", piece, sizes)
        return (time.perf_counter() - t0) * 1e3

    def leg_n():
        f = files["n"]
        t0 = time.perf_counter()
        first = np.asarray([0, f["frames"].size], np.uintp)
        frames, cons = np.zeros(1, np.int64), np.zeros(1, np.uintp)
        rc = hlib.flake_amd_decode_set_index(g, n, f["frames"].ctypes.data, first.ctypes.data, 1, all_sizes.ctypes.data, cap_all,
                                             frames.ctypes.data, cons.ctypes.data)
        assert rc == 0 and frames[0] == NF and cons[0] == f["frames"].size, hlib.flake_amd_decode_set_last_error(g)
        window("n", f["frames"], all_sizes[:NF])
        return (time.perf_counter() - t0) * 1e3

    ms = {"t": [], "n": []}
    for r in range(rounds + 1):
        for k, fn in (("t", leg_t), ("n", leg_n)):
            v = fn()
            if r:
                ms[k].append(v)
    hlib.flake_amd_decode_set_close(g)
    assert np.array_equal(out["t"], out["n"])
    npts = V.read_seektable(files["t"]["table"])[1]
    sec = [f"{SEEK_MARK}{NF} frames of {n} ({files['n']['frames'].size} bytes of frames), written by flake_amd_cli with --seekpoints "
           f"{SPACING} ({npts} points) and without; one window of {WIN} samples from sample {SKIP}; index + "
           f"flake_amd_decode_set_windows, medians of {rounds} after one discarded, {torch.cuda.get_device_name(0)}:"]
    for k, what in (("t", "SEEKTABLE: the piece between two points indexed on the CPU"),
                    ("n", "no table: the whole file indexed on the device (K8)")):
        v = ms[k]
        sec.append(f"  {k}  {what:62s} {indexed[k][0]:5d} frames indexed, {indexed[k][1]} decoded {statistics.median(v):9.2f} ms  "
                   f"(min {min(v):.2f}, max {max(v):.2f})")
    return sec


if SEEK_ONLY:
    sec = seek_leg()
    print("\n".join(sec), flush=True)
    old = open(out_path).read().split("\n") if os.path.exists(out_path) else []
    cut = next((i for i, ln in enumerate(old) if ln.startswith(SEEK_MARK)), len(old))
    kept = old[:cut]
    while kept and not kept[-1]:
        kept.pop()
    open(out_path, "w").write("\n".join(kept + [""] + sec) + "\n")
    sys.exit(0)

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
say()
for ln in seek_leg():
    say(ln)
open(out_path, "w").write("\n".join(lines) + "\n")
