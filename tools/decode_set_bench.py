"""Decode sets against one decoder per stream: the project's headline batch -- 4096 stereo 16-bit frames of 4096
samples, level 5 -- decoded as one stream, as 256 streams of 16 frames and as 16 streams of 256, through
flake_amd.HostDecoder (one after another) and through flake_amd.DecodeSet (one call) with the MD5 on the device and
on the host.  One process, the legs alternating, the first round discarded, medians of the rest with their spread.
Then the kernels alone: k_md5_ranges beside k_md5_streams' fast path on the same bytes (per-lane MB/s), and K7 with and
without a segment table.  Writes profiles/decode_set_bench.txt.
    python tools/decode_set_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "decode_set_bench.txt")
NF, n, ch = 4096, 4096, 2
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


pcm = np.ascontiguousarray(V.synth_pcm(NF, n, ch, 16).reshape(NF, n * ch), np.int32)
p = V.level_params(5, block_size=n, variable_block_size=0)
si = V.HostStreaminfo(min_block_size=n, max_block_size=n, sample_rate=44100, channels=ch, bits_per_sample=16)


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


SWEEP = [1, 2, 4, 8, 16, 32, 64, 256]
with V.Encoder(p, max_frames=NF) as enc:
    data = {S: encode_streams(enc, S) for S in SWEEP}
want16 = pcm.astype(np.int16).reshape(-1, ch)


outbuf = np.ones((NF * n, ch), np.int16)                  # touched: no page faults in the timed calls
hlib = V.load_host_library()
CALLS = {}
for S in SWEEP:
    CALLS[S] = dict(sor=np.arange(S, dtype=np.int32), fof=np.full(S, NF // S, np.int32),
                    st=np.ascontiguousarray(np.concatenate([d[0] for d in data[S]])),
                    sizes=np.ascontiguousarray(np.concatenate([d[1] for d in data[S]])), rs=np.zeros(S, np.int64))
md5buf = (C.c_ubyte * 16)()


def leg_decoders(S, with_open):
    """One decoder per stream (flake_amd_decode_*), one after another, each into its part of one output buffer; returns
    (ms with open and close, ms inside decode_frames + md5 alone)."""
    t0 = time.perf_counter()
    inner = 0.0
    per = NF // S * n
    for s, (st, fb) in enumerate(data[S]):
        d = hlib.flake_amd_decode_open(C.byref(si))
        t1 = time.perf_counter()
        got = hlib.flake_amd_decode_frames(d, st.ctypes.data, st.size, fb.ctypes.data, len(fb),
                                           outbuf[s * per:].ctypes.data, 2, per)
        assert got == per and hlib.flake_amd_decode_md5(d, md5buf) == 0
        inner += time.perf_counter() - t1
        hlib.flake_amd_decode_close(d)
    return (time.perf_counter() - t0) * 1e3, inner * 1e3


def leg_set(S, flags):
    """All streams through one decode set in ONE call, then every digest; the set is opened outside the timed part
    (a set serves a whole folder; leg b' gives the decoders the same allowance)."""
    g = hlib.flake_amd_decode_set_open(C.byref(si), S, flags)
    c = CALLS[S]
    t0 = time.perf_counter()
    got = hlib.flake_amd_decode_set_frames(g, S, c["sor"].ctypes.data, c["fof"].ctypes.data, c["st"].ctypes.data, c["st"].size,
                                           c["sizes"].ctypes.data, outbuf.ctypes.data, 2, NF * n, c["rs"].ctypes.data)
    if not flags & V.SET_MD5_OFF:
        for s in range(S):
            assert hlib.flake_amd_decode_set_md5(g, s, md5buf) == 0
    dt = (time.perf_counter() - t0) * 1e3
    assert got == NF * n and hlib.flake_amd_decode_set_device_batches(g) == 4      # (4M samples per device batch)
    hlib.flake_amd_decode_set_close(g)
    return dt


legs = {
    "a  1 stream, HostDecoder": lambda: leg_decoders(1, True)[1],
    "b  256 streams x 16, one HostDecoder each (open + decode + md5 + close)": lambda: leg_decoders(256, True)[0],
    "b' the same, decode + md5 calls alone": lambda: leg_decoders(256, True)[1],
    "c  256 streams x 16, DecodeSet, device MD5": lambda: leg_set(256, 0),
    "d  256 streams x 16, DecodeSet, FLAKE_AMD_SET_MD5_HOST": lambda: leg_set(256, V.SET_MD5_HOST),
    "e  16 streams x 256, DecodeSet, device MD5": lambda: leg_set(16, 0),
    "e' 16 streams x 256, DecodeSet, FLAKE_AMD_SET_MD5_HOST": lambda: leg_set(16, V.SET_MD5_HOST),
    "f  1 stream, DecodeSet, device MD5": lambda: leg_set(1, 0),
    "f' 1 stream, DecodeSet, FLAKE_AMD_SET_MD5_HOST": lambda: leg_set(1, V.SET_MD5_HOST),
    "o  256 streams x 16, DecodeSet, FLAKE_AMD_SET_MD5_OFF": lambda: leg_set(256, V.SET_MD5_OFF),
}
ms = {k: [] for k in legs}
for r in range(rounds + 1):
    print(f"legs, round {r}", file=sys.stderr, flush=True)
    for k, fn in legs.items():
        v = fn()
        if r:
            ms[k].append(v)
say(f"{NF} stereo 16-bit frames of {n}, level 5, FLAKE_AMD_BATCH={NF}, int16 output; {rounds} timed rounds after one "
    f"discarded, legs alternating; {torch.cuda.get_device_name(0)}")
med = {}
for k, v in ms.items():
    med[k[:2].strip()] = statistics.median(v)
    say(f"  {k}: median {statistics.median(v):.1f} ms (min {min(v):.1f}, max {max(v):.1f})")


def ratio(x, y):
    a, b = ms[[k for k in ms if k[:2].strip() == x][0]], ms[[k for k in ms if k[:2].strip() == y][0]]
    rs = sorted(u / w for u, w in zip(a, b))
    return f"{statistics.median(rs):.2f} (per round {rs[0]:.2f} .. {rs[-1]:.2f})"


say(f"  b / c = {ratio('b', 'c')};  b' / c = {ratio(chr(98) + chr(39), 'c')};  a / c = {ratio('a', 'c')};  a - c = "
    f"{med['a'] - med['c']:.1f} ms;  d - c = {med['d'] - med['c']:.1f} ms;  e - e' = {med['e'] - med[chr(101) + chr(39)]:.1f} ms")

# where the device hash starts to win: both MD5 legs for every stream count
say("device MD5 against FLAKE_AMD_SET_MD5_HOST by stream count (median ms of the same rounds):")
sweep = {(S, f): [] for S in SWEEP for f in (0, V.SET_MD5_HOST)}
for r in range(rounds + 1):
    print(f"sweep, round {r}", file=sys.stderr, flush=True)
    for key in sweep:
        v = leg_set(*key)
        if r:
            sweep[key].append(v)
for S in SWEEP:
    d, h = statistics.median(sweep[(S, 0)]), statistics.median(sweep[(S, V.SET_MD5_HOST)])
    say(f"  {S:4d} streams: device {d:7.1f} ms (min {min(sweep[(S, 0)]):.1f}, max {max(sweep[(S, 0)]):.1f}), host {h:7.1f} ms "
        f"(min {min(sweep[(S, V.SET_MD5_HOST)]):.1f}, max {max(sweep[(S, V.SET_MD5_HOST)]):.1f}): "
        f"{'device' if d < h else 'host'} wins by {abs(d - h):.1f} ms")

# ---- the kernels alone ----------------------------------------------------------------------------
dev = torch.device("cuda", 0)


def timed(fn, reps=5):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])


say("K6 alone, the whole batch's int16 PCM on the device (67 MB), S streams of equal length, one lane each:")
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_pcm_format(V.PCM_S16)
    stream = torch.cuda.Stream()
    enc.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        dpcm = torch.from_numpy(np.concatenate([want16.reshape(-1), np.zeros(64, np.int16)])).to(dev)
        for S in (16, 256):
            per = NF // S
            states = torch.zeros(S * V.MD5_STATE_BYTES, dtype=torch.uint8, device=dev)
            first = torch.arange(0, S + 1, dtype=torch.int32, device=dev)
            rng = torch.arange(0, S, dtype=torch.int32, device=dev)
            bfirst = (torch.arange(0, S + 1, dtype=torch.int32) * per).to(dev)
            blocks = torch.arange(0, NF, dtype=torch.int32, device=dev)
            lens = torch.full((S,), per * n, dtype=torch.int64, device=dev)
            mb = per * n * ch * 2 / 1e6
            res = {}
            for name, shift in (("aligned", 0), ("one sample on (4-byte aligned)", 1)):
                starts = (torch.arange(0, S, dtype=torch.int64) * per * n + shift).to(dev)
                stream.synchronize()
                enc.md5_init_dev(states, S)
                t = timed(lambda: enc.md5_update_ranges_dev(states, S, dpcm, first, rng, starts, lens))
                assert enc.last_launches() == ["k_md5_ranges<int16_t,2>"]
                say(f"  {S:3d} streams, k_md5_ranges, starts {name}: {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}) = "
                    f"{mb / t[0] * 1e3:.0f} MB/s per lane")
            enc.md5_init_dev(states, S)
            t = timed(lambda: enc.md5_update_dev(states, S, dpcm, n, bfirst, blocks))
            assert enc.last_launches()[-1].endswith("fast")
            say(f"  {S:3d} streams, k_md5_streams fast path (with k_md5_scan): {t[0]:.2f} ms (min {t[1]:.2f}, max {t[2]:.2f}) = "
                f"{mb / t[0] * 1e3:.0f} MB/s per lane")
    enc.set_stream(None)

say("K7 alone (fhip_set_profiling: k_decode_frames + k_decode + k_decode_final [+ k_decode_seg_final]), the host entry:")
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_pcm_format(V.PCM_S16)
    enc.set_profiling(True)
    out = np.zeros((NF * n, ch), np.int16)
    for S in (1, 16, 256):
        st = np.concatenate([d[0] for d in data[S]])
        fb = np.concatenate([d[1] for d in data[S]])
        sf = np.arange(0, S + 1, dtype=np.int32) * (NF // S)
        ts = []
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            res = enc.decode_frames_segments(st, fb, NF * n, sf, np.zeros(S, np.int64), out=out)
            assert res[0] == V.OK
            ts.append(enc.kernel_times(reset=True)["k_decode"][0])
        say(f"  {S:3d} segments: {statistics.median(ts[1:]):.2f} ms (min {min(ts[1:]):.2f}, max {max(ts[1:]):.2f})")
    st, fb = data[1][0]
    ts = []
    for r in range(rounds + 1):
        enc.kernel_times(reset=True)
        assert enc.decode_frames(st, fb, NF * n, False, 0, out=out)[0]
        ts.append(enc.kernel_times(reset=True)["k_decode"][0])
    say(f"  no table (fhip_decode_frames, one stream): {statistics.median(ts[1:]):.2f} ms (min {min(ts[1:]):.2f}, max {max(ts[1:]):.2f})")

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
