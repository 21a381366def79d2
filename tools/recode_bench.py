"""Recode sets against the two-step path: the headline decode batch -- 4096 stereo 16-bit frames of 4096 samples, level 5,
as 256 streams of 16 frames -- re-encoded at levels 5, 8 and 10 (variable block size)
  r  through one flake_amd.RecodeSet (the PCM stays on the device, one hash),
  t  through flake_amd.DecodeSet to host memory, re-cut into the encoder's blocks in numpy, then flake_amd.StreamSet from
     host memory with its device MD5 (int16 samples where the set takes them: levels 5 and 8).
One process, the legs alternating, the first round discarded, medians of the rest with their spread; the sets are opened
outside the timed part.  The two legs' bytes are compared in the discarded round.  Then k_gather_spans alone
(fhip_set_profiling).  No threshold is asserted.  Writes profiles/recode_bench.txt.
    python tools/recode_bench.py [timed rounds] [output file]"""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch, flake_amd

V = flake_amd
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "recode_bench.txt")
NF, n, ch, S = 4096, 4096, 2, 256
PER = NF // S
os.environ["FLAKE_AMD_BATCH"] = str(NF)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


pcm = np.ascontiguousarray(V.synth_pcm(NF, n, ch, 16).reshape(NF, n * ch), np.int32)
si = V.HostStreaminfo(min_block_size=n, max_block_size=n, sample_rate=44100, channels=ch, bits_per_sample=16)
data = []
with V.Encoder(V.level_params(5, block_size=n, variable_block_size=0), max_frames=NF) as enc:
    for s in range(S):
        part = pcm[s * PER:(s + 1) * PER]
        fb = np.zeros(PER, np.int32)
        b = V.Batch()
        b.pcm, b.nframes, b.block_size, b.frame_bytes, b.first_frame_number = part.ctypes.data, PER, n, fb.ctypes.data, 0
        cap = PER * enc.frame_stride(n) + 64
        buf = np.zeros(cap, np.uint8)
        wrote = C.c_int64(0)
        assert enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), buf.ctypes.data, cap, C.byref(wrote)) == 0
        data.append((buf[:wrote.value].copy(), fb))
runs = [(s, data[s][0], data[s][1]) for s in range(S)]
samples = PER * n                                       # per stream


def leg_recode(level, flags):
    with V.RecodeSet(si, S, level=level, flags=flags) as rs:
        t0 = time.perf_counter()
        blocks = rs.recode_runs(runs) + rs.finish()
        infos = [rs.streaminfo_bytes(s) for s in range(S)]
        dt = (time.perf_counter() - t0) * 1e3
        batches = rs.device_batches()
    out = [b""] * S
    for s, d in blocks:
        out[s] += d
    return dt, out, infos, batches


def leg_two_step(level, flags):
    narrow = not flags & V.SET_VBS
    with V.DecodeSet(si, S) as ds, V.StreamSet(S, level=level, flags=flags) as st:
        bs = st.block_size
        t0 = time.perf_counter()
        got = ds.decode_runs(runs, S * samples, 2 if narrow else 4)
        digests = [ds.md5(s) for s in range(S)]                          # (the decode side's check of the source)
        # the decoder's blocks re-cut into the encoder's, per stream: whole blocks round-robin, then the tails
        nb, tail = samples // bs, samples % bs
        out = [b""] * S
        if nb:
            whole = np.ascontiguousarray(np.stack([g[:nb * bs].reshape(nb, bs * ch) for g in got], axis=1))
            frames, sizes = st.encode(whole, bs, np.tile(np.arange(S, dtype=np.int32), nb), dtype=whole.dtype)
            at = 0
            for k, z in enumerate(sizes):
                out[k % S] += frames[at:at + z].tobytes()
                at += z
        if tail:
            tails = np.ascontiguousarray(np.concatenate([g[nb * bs:] for g in got]))
            frames, sizes = st.encode_ragged(tails, [tail] * S, np.arange(S, dtype=np.int32), dtype=tails.dtype)
            at = 0
            for k, z in enumerate(sizes):
                out[k] += frames[at:at + z].tobytes()
                at += z
        infos = [st.streaminfo_bytes(s) for s in range(S)]
        dt = (time.perf_counter() - t0) * 1e3
        assert all(d is not None for d in digests)
    return dt, out, infos


LEVELS = [(5, 0), (8, 0), (10, V.SET_VBS)]
ms = {(k, lv): [] for lv, _ in LEVELS for k in "rt"}
for r in range(rounds + 1):
    print(f"round {r}", file=sys.stderr, flush=True)
    for lv, fl in LEVELS:
        a = leg_recode(lv, fl)
        b = leg_two_step(lv, fl)
        if r == 0:
            assert a[1] == b[1] and a[2] == b[2], f"level {lv}: the two legs' bytes differ"
            say(f"level {lv}: {sum(map(len, a[1]))} bytes out, identical from both legs, STREAMINFO included; "
                f"recode set: {a[3][0]} decode and {a[3][1]} encode batches")
        else:
            ms[("r", lv)].append(a[0])
            ms[("t", lv)].append(b[0])
say(f"{S} streams of {PER} stereo 16-bit frames of {n} (level 5) re-encoded; FLAKE_AMD_BATCH={NF}; {rounds} timed rounds after "
    f"one discarded, legs alternating; {torch.cuda.get_device_name(0)}")
for lv, _ in LEVELS:
    r_, t_ = ms[("r", lv)], ms[("t", lv)]
    ratios = sorted(t / r for t, r in zip(t_, r_))
    say(f"  level {lv:2d}: RecodeSet median {statistics.median(r_):.1f} ms (min {min(r_):.1f}, max {max(r_):.1f}); "
        f"DecodeSet + StreamSet median {statistics.median(t_):.1f} ms (min {min(t_):.1f}, max {max(t_):.1f}); "
        f"two-step / recode = {statistics.median(ratios):.2f} (per round {ratios[0]:.2f} .. {ratios[-1]:.2f})")

# ---- k_gather_spans alone ---------------------------------------------------------------------------
say("k_gather_spans alone (fhip_set_profiling), the batch's int32 PCM on the device (134 MB read, 134 MB written):")
dev = torch.device("cuda", 0)
with V.Encoder(V.level_params(5, block_size=n, variable_block_size=0), max_frames=8) as enc:
    enc.set_profiling(True)
    src = torch.from_numpy(pcm.reshape(-1, ch)).to(dev)
    carry = torch.zeros((S * n, ch), dtype=torch.int32, device=dev)
    dst = torch.zeros((NF * n + 8, ch), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    total = NF * n
    tables = {
        "4096 pieces of 4096 samples, stream by stream (a recode step's table)":
            [(1, ((k % PER) * S + k // PER) * n, k * n, n) for k in range(NF)],
        "the same, every destination one sample on (source and destination disagree modulo 16 bytes)":
            [(0, 0, 0, 1)] + [(1, ((k % PER) * S + k // PER) * n, 1 + k * n, n) for k in range(NF)],
        "one piece": [(1, 0, 0, total)],
        "1048576 pieces of 32 samples": [(1, ((k * 7919) % (total // 32)) * 32, k * 32, 32) for k in range(total // 32)],
    }
    for name, rows in tables.items():
        t = V.gather_pieces(rows)
        ts = []
        for r in range(rounds + 1):
            enc.kernel_times(reset=True)
            assert enc.gather_spans_dev(dst, NF * n + 8, carry, S * n, src, total, t) == V.OK
            enc.sync()
            ts.append(enc.kernel_times(reset=True)["k_gather_spans"][0])
        moved = sum(c for *_, c in rows) * ch * 4 * 2 / 1e9
        say(f"  {name}: {statistics.median(ts[1:]):.3f} ms (min {min(ts[1:]):.3f}, max {max(ts[1:]):.3f}) = "
            f"{moved / statistics.median(ts[1:]) * 1e3:.0f} GB/s read + written")

os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
