"""Encode rows from the device against the composition a caller had before: the shapes of tools/decode_rows_bench.py --
256 and 4096 rows of 4096 stereo 16-bit samples as a float32 tensor [R][2][4096] on the device, every row a stream of
its own and one block of 4096, level 5, each stream's MD5 on the device.
  r  flake_amd_set_encode_rows from the tensor (the current stream synchronised first, as StreamSet.encode_rows does)
  c  torch scale / round / clamp / permute to interleaved int16, download, flake_amd_set_encode (int16 samples, the
     cheapest form the host entry takes; no row has a short block, so flake_amd_set_encode_ragged has nothing to do)
The composition uses only entries the project had before, so it is the baseline.  Both legs write into a buffer made
before the clock starts and end with the bytes on the host; the bytes and every stream's STREAMINFO are compared in the
discarded round.  One process, the legs alternating, medians of the timed rounds with min and max.  Then K12 beside the
encode kernels (fhip_set_profiling) through fhip_frames_packed_from_rows + fhip_frames_packed_begin, one batch.
Writes profiles/encode_rows_bench.txt.
    python tools/encode_rows_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "encode_rows_bench.txt")
NF, n, ch = 4096, 4096, 2
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


hlib = V.load_host_library()
dev = torch.device("cuda", 0)
# [NF][ch][n] float32 in [-1, 1), off the 16-bit grid so that the rounding has work to do
pcm = V.synth_pcm(NF, n, ch, 16).reshape(NF, n, ch).transpose(0, 2, 1)
noise = np.random.default_rng(7).uniform(-0.45, 0.45, size=pcm.shape)
all_rows = torch.from_numpy(np.ascontiguousarray((pcm + noise) / 32768.0, np.float32)).to(dev)
del noise


def open_set(S):
    ctx = V.HostContext(channels=ch, sample_rate=44100, bits_per_sample=16)
    ctx.params.compression = 5
    assert hlib.flake_amd_set_defaults(C.byref(ctx.params)) == 0
    ctx.params.block_size = n
    g = hlib.flake_amd_set_open(C.byref(ctx), S, 0)
    assert g, hlib.flake_amd_set_last_error(None)
    return g


def infos(g, S):
    out = []
    for s in range(S):
        si = V.HostStreaminfo()
        assert hlib.flake_amd_set_get_streaminfo(g, s, C.byref(si)) == 0
        out.append(V.write_streaminfo(si))
    return out


def case(S):
    return dict(S=S, rows=all_rows[:S], streams=np.arange(S, dtype=np.int32), lens=np.full(S, n, np.int64),
                out=np.zeros(S * (n * ch * 2 + n) + 4096, np.uint8), whole=np.zeros(S, np.int64), tail=np.zeros(S, np.int64),
                fs=np.zeros(S, np.int32), head=[])


def leg_r(c, check):
    g = open_set(c["S"])
    t0 = time.perf_counter()
    torch.cuda.current_stream(dev).synchronize()
    w = hlib.flake_amd_set_encode_rows(g, c["rows"].data_ptr(), V.ROWS_F32, c["S"], n, c["streams"].ctypes.data,
                                       c["lens"].ctypes.data, c["out"].ctypes.data, c["out"].size, c["whole"].ctypes.data,
                                       c["tail"].ctypes.data)
    dt = (time.perf_counter() - t0) * 1e3
    assert w > 0, hlib.flake_amd_set_last_error(g)
    res = (c["out"][:w].tobytes(), infos(g, c["S"])) if check else None
    hlib.flake_amd_set_close(g)
    return dt, res


def leg_c(c, check):
    g = open_set(c["S"])
    t0 = time.perf_counter()
    host = (c["rows"] * 32768.0).round().clamp(-32768.0, 32767.0).to(torch.int16).permute(0, 2, 1).contiguous().cpu().numpy()
    t1 = time.perf_counter()
    w = hlib.flake_amd_set_encode(g, host.ctypes.data, 2, c["S"], n, c["streams"].ctypes.data, c["out"].ctypes.data,
                                  c["out"].size, c["fs"].ctypes.data)
    t2 = time.perf_counter()
    assert w > 0, hlib.flake_amd_set_last_error(g)
    c["head"].append((t1 - t0) * 1e3)
    res = (c["out"][:w].tobytes(), infos(g, c["S"])) if check else None
    hlib.flake_amd_set_close(g)
    return (t2 - t0) * 1e3, res


say(f"rows of {n} stereo 16-bit samples as float32 [R][{ch}][{n}] on the device, one stream and one block of {n} per row, level 5, "
    f"device MD5; FLAKE_AMD_BATCH={NF}; {rounds} timed rounds after one discarded, legs alternating; {torch.cuda.get_device_name(0)}")
for S in (256, NF):
    c = case(S)
    ms = {"r": [], "c": []}
    for r in range(rounds + 1):
        print(f"{S} rows, round {r}", file=sys.stderr, flush=True)
        got = {}
        for k, fn in (("r", leg_r), ("c", leg_c)):
            v, got[k] = fn(c, r == 0)
            if r:
                ms[k].append(v)
        if r == 0:
            assert got["r"][0] == got["c"][0] and got["r"][1] == got["c"][1], "the legs' bytes or STREAMINFOs differ"
            nbytes = len(got["r"][0])
            c["head"] = []
        del got
    say()
    say(f"{S} rows ({S * n * ch * 4 / 1e6:.1f} MB of float32 in, {nbytes / 1e6:.1f} MB of FLAC out, equal in both legs):")
    for k, what in (("r", "flake_amd_set_encode_rows from the float32 tensor"),
                    ("c", "torch scale, round, clamp, permute -> int16, download, flake_amd_set_encode")):
        v = ms[k]
        say(f"  {k}  {what:78s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
    say(f"     of c, before the encode call (the torch kernels and the download): {statistics.median(c['head']):.2f} ms")
    say("  c / r per round: " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["c"], ms["r"])))

say()
say('K12 beside the encode kernels (fhip_set_profiling), fhip_frames_packed_from_rows + fhip_frames_packed_begin on one batch, '
    f"medians of {rounds}:")
p = V.level_params(5, block_size=n, variable_block_size=0)
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_profiling(True)
    for S in (256, NF):
        pieces = V.row_pieces([(r, 0, r * n, n) for r in range(S)])
        fb = np.zeros(S, np.int32)
        times = {}
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            assert enc.frames_packed_from_rows(0x1000, S, n, all_rows[:S], S, n, V.ROWS_F32, pieces) == V.OK
            b = V.Batch(pcm=0x1000, nframes=S, block_size=n, frame_bytes=fb.ctypes.data, first_frame_number=0)
            total = C.c_int64(0)
            assert enc.lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total)) == V.OK
            buf = np.zeros(int(total.value), np.uint8)
            assert enc.lib.fhip_frames_packed_fetch(enc._h, buf.ctypes.data, buf.size) == V.OK
            enc.sync()
            kt = enc.kernel_times(reset=True)
            if r:
                for k, (t, cnt) in kt.items():
                    if cnt:
                        times.setdefault(k, []).append(t)
        k12 = statistics.median(times.pop("k_rows_to_pcm"))
        say(f"  {S:5d} rows: k_rows_to_pcm {k12:7.3f} ms ({S * n * ch * 8 / k12 / 1e6:.0f} GB/s of float32 read and int32 written);  "
            + "  ".join(f"{k} {statistics.median(v):.3f}" for k, v in sorted(times.items())))
open(out_path, "w").write("\n".join(lines) + "\n")
