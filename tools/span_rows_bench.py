"""Span rows against the composition they replace: tools/held_bench.py's shapes -- 4096 stereo 16-bit frames of 4096
samples, level 5, as 256 streams of 16 frames, all held; then the many-files case, 4096 streams (the 256 streams' bytes
sixteen times over).  Every stream is walked whole, twice:
  chunks    (row_len, hop) = (4096, 4096) from sample 100 on: plain chunking that is not aligned to the blocks
  overlap   (row_len, hop) = (4096, 2048) from sample 0 on: half-overlapping rows
  s   DecodeSet.held_span_rows: one span per stream, every frame decoded once, K13 lays the rows
  w   DecodeSet.held_windows_rows over the equivalent windows (id, first + j * hop, min(row_len, count - j * hop)): one
      window per row, K10 lays them
float32 rows [R][2][4096].  One set holds the streams; each call allocates its rows with torch.empty and ends
synchronised.  One process, the legs interleaved round by round, medians of the timed rounds with min and max, the ratio
w / s per round, both legs' frames_decoded; the two tensors and the lengths are compared for equality in the discarded
round.  Then the kernels alone (fhip_set_profiling: "k_decode" is K7's header pass, frame pass and ends; "k_span_rows",
"k_window_rows") through fhip_decode_frames_windows_spans_held and fhip_decode_frames_windows_rows_held, 64 streams a
call.  Writes profiles/span_rows_bench.txt.
    python tools/span_rows_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "span_rows_bench.txt")
NF, n, ch, PER = 4096, 4096, 2, 16
S0, TOTAL = NF // PER, PER * n
SHAPES = (("chunks", 4096, 4096, 100), ("overlap", 4096, 2048, 0))      # name, row_len, hop, the span's first sample
GROUP = 64                                                             # streams per call of the kernels-alone part
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


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


def case(mult):
    S = S0 * mult
    c = dict(S=S, st=np.ascontiguousarray(np.tile(np.concatenate([d[0] for d in data]), mult)),
             sizes=np.ascontiguousarray(np.tile(np.concatenate([d[1] for d in data]), mult)))
    streams = [data[s % S0][0] for s in range(S)]
    c["g"] = V.DecodeSet(si, 1, V.SET_MD5_OFF)
    c["g"].hold(c["st"].size)
    ids = []
    for a in range(0, S, S0):
        ids += c["g"].hold_add(streams[a:a + S0], fixed_block_sizes=[n] * S0, max_block_size=n)
    c["ids"] = ids
    assert c["g"].held_stats()[:2] == (c["st"].size, S * PER)
    return c


def rows_of(row_len, hop, first):
    """(R, [(first sample, count)] per row) of one stream's span."""
    count = TOTAL - first
    R = V.span_rows_count(count, row_len, hop)
    return R, [(first + j * hop, min(row_len, count - j * hop)) for j in range(R)]


def leg_s(c, row_len, hop, first):
    spans = [(i, first, TOTAL - first) for i in c["ids"]]
    t0 = time.perf_counter()
    rows, lens, _, status, decoded = c["g"].held_span_rows(spans, row_len, hop, torch.float32)
    dt = (time.perf_counter() - t0) * 1e3
    assert not status.any()
    return dt, rows, lens, decoded


def leg_w(c, row_len, hop, first):
    per = rows_of(row_len, hop, first)[1]
    wins = [(i, a, m) for i in c["ids"] for a, m in per]
    t0 = time.perf_counter()
    rows, lens, status, decoded = c["g"].held_windows_rows(wins, row_len, torch.float32)
    dt = (time.perf_counter() - t0) * 1e3
    assert not status.any()
    return dt, rows, lens, decoded


LEGS = (("s", leg_s, "DecodeSet.held_span_rows, one span per stream"), ("w", leg_w, "DecodeSet.held_windows_rows, one window per row"))
say(f"{NF} stereo 16-bit frames of {n}, level 5, as held streams of {PER} frames, every stream walked whole; float32 rows; "
    f"FLAKE_AMD_BATCH={NF}; {rounds} timed rounds after one discarded, legs interleaved; {torch.cuda.get_device_name(0)}")
cases = {}
for mult in (1, 16):
    c = cases[mult] = case(mult)
    for name, row_len, hop, first in SHAPES:
        ms, decoded = {k: [] for k, _, _ in LEGS}, {}
        for r in range(rounds + 1):
            print(f"{c['S']} streams, {name}, round {r}", file=sys.stderr, flush=True)
            got = {}
            for k, fn, _ in LEGS:
                v, rows, lens, decoded[k] = fn(c, row_len, hop, first)
                if r:
                    ms[k].append(v)
                else:
                    got[k] = (rows, lens)
                del rows
            if r == 0:
                assert torch.equal(got["s"][0], got["w"][0]) and torch.equal(got["s"][1], got["w"][1]) and bool(got["s"][0].any())
                nrows = got["s"][0].shape[0]
            del got
        say()
        say(f"{c['S']} streams, {name}: row_len {row_len}, hop {hop}, from sample {first}; {nrows} rows "
            f"({nrows * ch * row_len * 4 / 1e6:.0f} MB); frames handed to the device: s {decoded['s']}, w {decoded['w']} "
            f"of {c['S'] * PER} in the streams; the rows and lengths of both legs are equal")
        for k, _, what in LEGS:
            v = ms[k]
            say(f"  {k:2s}  {what:60s} {statistics.median(v):9.2f} ms  (min {min(v):.2f}, max {max(v):.2f})")
        say("  w / s per round: " + " ".join(f"{a / b:.2f}" for a, b in zip(ms["w"], ms["s"])))

say()
say('The kernels alone (fhip_set_profiling: "k_decode" is the header pass, the frame pass and the ends), '
    f"fhip_decode_frames_windows_spans_held and fhip_decode_frames_windows_rows_held, {GROUP} streams a call, medians of {rounds}:")
with V.Encoder(p, max_frames=NF) as enc:
    enc.set_profiling(True)
    for mult in (1, 16):
        c = cases[mult]
        store = torch.from_numpy(c["st"]).to(dev)
        off = np.concatenate([[0], np.cumsum(c["sizes"])]).astype(np.int64)
        for name, row_len, hop, first in SHAPES:
            R, per = rows_of(row_len, hop, first)
            rows = torch.empty((c["S"] * R, ch, row_len), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            # a group's tables, relative to its first stream: the span leg takes every frame once, the window leg each
            # window's frames
            wf = [(a // n, (a + m - 1) // n, a - (a // n) * n, m) for a, m in per]
            t = {"s": ([], []), "w": ([], [])}
            for r in range(rounds + 1):
                for leg in ("s", "w"):
                    enc.kernel_times(reset=True)
                    for a in range(0, c["S"], GROUP):
                        g = min(GROUP, c["S"] - a)
                        if leg == "s":
                            res = enc.decode_frames_windows_spans_held(
                                store, c["st"].size, off[a * PER:(a + g) * PER], c["sizes"][a * PER:(a + g) * PER], g * TOTAL,
                                np.arange(g + 1) * PER, [first] * g, [TOTAL - first] * g, (a + np.arange(g)) * R, [R] * g,
                                np.zeros(g, np.int64), hop, rows, c["S"] * R, row_len, V.ROWS_F32, seg_number=[0] * g)
                        else:
                            fr = np.concatenate([np.arange((a + w) * PER + f0, (a + w) * PER + f1 + 1)
                                                 for w in range(g) for f0, f1, _, _ in wf])
                            sf = np.concatenate([[0], np.cumsum([f1 - f0 + 1 for f0, f1, _, _ in wf] * g)])
                            res = enc.decode_frames_windows_rows_held(
                                store, c["st"].size, off[fr], c["sizes"][fr], g * sum(m for _, m in per), sf,
                                [sk for _, _, sk, _ in wf] * g, [m for _, _, _, m in wf] * g, a * R + np.arange(g * R),
                                np.zeros(g * R, np.int64), rows, c["S"] * R, row_len, V.ROWS_F32,
                                seg_number=[f0 for f0, _, _, _ in wf] * g)
                        assert res[0] == V.OK, res[-1]
                    kt = enc.kernel_times(reset=True)
                    if r:
                        t[leg][0].append(kt["k_decode"][0])
                        t[leg][1].append(kt["k_span_rows" if leg == "s" else "k_window_rows"][0])
            say(f"  {c['S']:5d} streams, {name:7s}: s  k_decode {statistics.median(t['s'][0]):8.3f} ms, k_span_rows "
                f"{statistics.median(t['s'][1]):7.3f} ms;   w  k_decode {statistics.median(t['w'][0]):8.3f} ms, k_window_rows "
                f"{statistics.median(t['w'][1]):7.3f} ms")
            del rows
        del store
for c in cases.values():
    c["g"].close()
open(out_path, "w").write("\n".join(lines) + "\n")
