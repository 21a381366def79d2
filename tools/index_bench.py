"""Frame discovery on one CPU core against K8 on the device: the project's headline decode batch -- 4096 stereo 16-bit
frames of 4096 samples, level 5 -- as one stream and as 256 streams of 16 frames.  One process, the legs alternating,
the first round discarded, medians of the rest with their spread.
  a  flake_amd_index_frames on one core (the yardstick: the code the CLI ran before K8)
  b  K8's launches alone, hipEvents around each (fhip_set_profiling), inside the host entry
  c  fhip_index_frames: upload, the launches, download, one wait
  d  256 streams: one call with 256 ranges against 256 calls of one range
  e  a whole set decode with discovery in it: index + flake_amd_decode_set_frames + every digest, indexed on the CPU
     against indexed on the device
Every device answer is compared with the CPU's before anything is timed.  Writes profiles/index_bench.txt.
    python tools/index_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "index_bench.txt")
NF, n, ch = 4096, 4096, 2
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


pcm = np.ascontiguousarray(V.synth_pcm(NF, n, ch, 16).reshape(NF, n * ch), np.int32)
p = V.level_params(5, block_size=n, variable_block_size=0)
si = V.HostStreaminfo(min_block_size=n, max_block_size=n, sample_rate=44100, channels=ch, bits_per_sample=16)
hlib = V.load_host_library()


def encode_streams(enc, S):
    """The batch as S streams of NF / S frames, each numbered from 0: [(bytes, sizes)]."""
    per, res = NF // S, []
    for s in range(S):
        part = pcm[s * per:(s + 1) * per]
        fb = np.zeros(per, np.int32)
        b = V.Batch()
        b.pcm, b.nframes, b.block_size, b.frame_bytes, b.first_frame_number = part.ctypes.data, per, n, fb.ctypes.data, 0
        cap = per * enc.frame_stride(n) + 64
        buf = np.zeros(cap, np.uint8)
        wrote = C.c_int64(0)
        assert enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), buf.ctypes.data, cap, C.byref(wrote)) == 0
        res.append((buf[:wrote.value].copy(), fb))
    return res


SHAPES = (1, 256)
with V.Encoder(p, max_frames=NF) as enc:
    data = {S: encode_streams(enc, S) for S in SHAPES}
CALL = {}
for S in SHAPES:
    st = np.ascontiguousarray(np.concatenate([d[0] for d in data[S]]))
    first = np.zeros(S + 1, np.int64)
    first[1:] = np.cumsum([d[0].size for d in data[S]])
    CALL[S] = dict(st=st, first=first, first_sz=first.astype(np.uintp), sizes=np.concatenate([d[1] for d in data[S]]),
                   fb=np.zeros(NF + 8, np.int32), fr=np.zeros(S, np.int32), co=np.zeros(S, np.int64), va=np.zeros(S, np.int32),
                   frames64=np.zeros(S, np.int64), cons=np.zeros(S, np.uintp),
                   sor=np.arange(S, dtype=np.int32), fof=np.full(S, NF // S, np.int32), rs=np.zeros(S, np.int64))
outbuf = np.ones((NF * n, ch), np.int16)
md5buf = (C.c_ubyte * 16)()
used = C.c_size_t(0)


def cpu_index(S):
    """flake_amd_index_frames over every stream of the shape, one after another; returns ms."""
    c = CALL[S]
    t0 = time.perf_counter()
    at = 0
    for s in range(S):
        lo, hi = int(c["first"][s]), int(c["first"][s + 1])
        k = hlib.flake_amd_index_frames(C.byref(si), c["st"][lo:].ctypes.data, hi - lo, c["fb"][at:].ctypes.data, NF - at,
                                        C.byref(used))
        assert k == NF // S and used.value == hi - lo
        at += k
    dt = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(c["fb"][:NF], c["sizes"])
    return dt


def dev_index(enc, S, lo_r=0, hi_r=None):
    """fhip_index_frames over ranges lo_r .. hi_r of the shape in one call; returns ms."""
    c = CALL[S]
    hi_r = S if hi_r is None else hi_r
    b0, b1 = int(c["first"][lo_r]), int(c["first"][hi_r])
    rf = c["first"][lo_r:hi_r + 1] - b0
    ii = V.IndexIn(c["st"][b0:].ctypes.data, b1 - b0, rf.ctypes.data, hi_r - lo_r, n, NF)
    io = V.IndexOut(c["fb"].ctypes.data, c["fr"].ctypes.data, c["co"].ctypes.data, c["va"].ctypes.data)
    t0 = time.perf_counter()
    rc = enc.lib.fhip_index_frames(enc._h, C.byref(ii), C.byref(io))
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == V.OK and np.all(c["fr"][:hi_r - lo_r] == NF // S)
    return dt


KNAMES = ("k_index_count", "k_index_wgscan", "k_index_scatter", "k_index_walk", "k_index_ranges", "k_index_emit")


def set_decode(S, on_device):
    """Discovery, the set's one decode call, every digest; the set is opened outside the timed part."""
    c = CALL[S]
    g = hlib.flake_amd_decode_set_open(C.byref(si), S, 0)
    t0 = time.perf_counter()
    if on_device:
        assert hlib.flake_amd_decode_set_index(g, n, c["st"].ctypes.data, c["first_sz"].ctypes.data, S, c["fb"].ctypes.data, NF,
                                               c["frames64"].ctypes.data, c["cons"].ctypes.data) == 0
    else:
        cpu_index(S)
    t1 = time.perf_counter()
    got = hlib.flake_amd_decode_set_frames(g, S, c["sor"].ctypes.data, c["fof"].ctypes.data, c["st"].ctypes.data, c["st"].size,
                                           c["fb"].ctypes.data, outbuf.ctypes.data, 2, NF * n, c["rs"].ctypes.data)
    for s in range(S):
        assert hlib.flake_amd_decode_set_md5(g, s, md5buf) == 0
    t2 = time.perf_counter()
    assert got == NF * n
    hlib.flake_amd_decode_set_close(g)
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3


with V.Encoder(p, max_frames=4) as enc:
    # the answers first
    for S in SHAPES:
        CALL[S]["fb"][:] = 0
        dev_index(enc, S)
        assert np.array_equal(CALL[S]["fb"][:NF], CALL[S]["sizes"]) and np.array_equal(CALL[S]["co"], np.diff(CALL[S]["first"]))
    ms = {}
    kt = {S: {k: [] for k in KNAMES} for S in SHAPES}

    def add(key, v, r):
        if r:
            ms.setdefault(key, []).append(v)

    for r in range(rounds + 1):
        print(f"round {r}", file=sys.stderr, flush=True)
        for S in SHAPES:
            add(f"a  {S:3d} streams, flake_amd_index_frames on one core", cpu_index(S), r)
            add(f"c  {S:3d} streams, fhip_index_frames, one call", dev_index(enc, S), r)
            enc.set_profiling(True)
            enc.kernel_times(reset=True)
            dev_index(enc, S)
            enc.sync()
            t = enc.kernel_times(reset=True)
            enc.set_profiling(False)
            if r:
                for k in KNAMES:
                    kt[S][k].append(t[k][0])
        t0 = time.perf_counter()
        for s in range(256):
            dev_index(enc, 256, s, s + 1)
        add("d  256 streams, 256 calls of one range", (time.perf_counter() - t0) * 1e3, r)
        for S in SHAPES:
            for on_device in (False, True):
                whole, disc = set_decode(S, on_device)
                tag = "device" if on_device else "CPU"
                add(f"e  {S:3d} streams, set decode with discovery on the {tag}", whole, r)
                add(f"e' {S:3d} streams, the discovery in it ({tag})", disc, r)

mb = {S: CALL[S]["st"].size / 1e6 for S in SHAPES}
say(f"{NF} stereo 16-bit frames of {n}, level 5 ({mb[1]:.1f} MB as one stream, {mb[256]:.1f} MB as 256); {rounds} timed rounds "
    f"after one discarded, legs alternating; {torch.cuda.get_device_name(0)}")
for k in sorted(ms):
    v = ms[k]
    say(f"  {k}: median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})")
for S in SHAPES:
    say(f"  b  {S:3d} streams, K8's launches alone (hipEvents, median ms; min .. max):")
    tot = [sum(kt[S][k][i] for k in KNAMES) for i in range(rounds)]
    for k in KNAMES:
        v = kt[S][k]
        say(f"       {k:16s} {statistics.median(v):7.3f}  ({min(v):.3f} .. {max(v):.3f})")
    say(f"       {'all six':16s} {statistics.median(tot):7.3f}  ({min(tot):.3f} .. {max(tot):.3f})  = "
        f"{mb[S] / statistics.median(tot):.1f} GB/s of stream")
for S in SHAPES:
    a, c = ms[f"a  {S:3d} streams, flake_amd_index_frames on one core"], ms[f"c  {S:3d} streams, fhip_index_frames, one call"]
    rs = sorted(x / y for x, y in zip(a, c))
    say(f"  a / c, {S} streams: {statistics.median(rs):.1f} (per round {rs[0]:.1f} .. {rs[-1]:.1f}); the CPU indexes "
        f"{mb[S] / statistics.median(a) * 1e3:.0f} MB/s; c's worst round {max(c):.2f} ms against a's best {min(a):.2f} ms")
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
