"""Diagnostic (not part of the product): cycles of the four consumer waves and the four producer waves of
k_autocorr_wt's workgroup 0 at the headline (configs[1]: 4096 stereo frames, n = 4096, LPC-8).
Consumers: the walk (the tile time is set by the slowest walk; the other waves wait for it at the next barrier),
the wait at the hand-over barriers and, of that, the wait for tile 0 (the cycles before the first walk).
Producers: staging (first conversion to last LDS store of a 128-position pass, summed; per row-pass = divided by
passes x rows), issuing the loads three or four passes ahead, and the wait at the barriers -- a producer that waits
as long as its consumer is not what the consumer waits for.  The SIMD of every wave (HW_ID) pairs them up.
The tile is 256 positions (128 steps per parity) in the long-tile form and 128 (64 steps) in the 128 form
(FHIP_WT_TILE=128 in the environment keeps the latter): fhip_autocorr_tile says which ran.
Needs the stamped build (add -DFHIP_PROBE_NOB for the probe that drops every b0 read, -DFHIP_PROBE_NOPROD /
-DFHIP_PROBE_NOLDSW for the ones that drop the staging / all but one of its LDS stores):
  python -c "from flake_amd.build import build_hip; build_hip(True, ['-DFHIP_STAMPS'], 'libflakehip_dbg.so')"
  FHIP_LIB=flake_amd/lib/libflakehip_dbg.so python tools/stamps_k1_waves.py [label [rows]]
rows: the build's producer split (FHIP_WT_ROWS_P0..3), e.g. 6,12,6,8; 8,8,8,8 when not given."""
import ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, flake_amd as fa
p = fa.level_params(5, order_method=fa.OM_MAX)
n = 4096; nfr = 4096
dev = torch.device("cuda", 0)
pcm = torch.from_numpy(fa.synth_pcm(nfr, n, 2, 16)).to(dev)
info = torch.zeros(nfr * 2 * fa.INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev)
enc = fa.Encoder(p, max_frames=nfr)
enc.set_stream(torch.cuda.current_stream().cuda_stream)
for _ in range(3):
    enc.encode_subframes_dev(pcm, nfr, n, info)
enc.sync()
st = (C.c_longlong * 64)()
# K1's own stamp array where the build exports it (its slots 40..63 are what fhip_debug_read_stamps passes on;
# a build that stamps k1_autocorr.hip alone has no other reader)
k1 = getattr(fa.load_library(), "fhip_debug_read_stamps_k1", None)
if k1 is not None:
    k1(st)
else:
    fa.load_library().fhip_debug_read_stamps(st)
groups = ["{0,2,4}", "{6,8}", "{1,3}", "{5,7}"]            # launch_autocorr's split at max order 8
lib = fa.load_library()
tile = lib.fhip_autocorr_tile(nfr * 2, n, 8) if hasattr(lib, "fhip_autocorr_tile") else 128   # (older builds: 128)
ntiles, steps = n // tile, tile // 2
rows = []
for w in range(4):
    walk, t0, bar, first = st[48 + w], st[52 + w], st[56 + w], st[60 + w]
    rows.append({"wave": w, "lags": groups[w], "walk_cycles": walk, "tile0_cycles": t0, "barrier_cycles": bar,
                 "first_wait_cycles": first,
                 "walk_cycles_per_step": round(walk / ((ntiles - 1) * steps), 2),
                 "barrier_cycles_per_handover": round(bar / ntiles, 1),
                 "later_barrier_cycles_per_handover": round((bar - first) / max(1, ntiles - 1), 1)})
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("FHIP_LIB", "libflakehip.so"))
split = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [8, 8, 8, 8]
slow = max(rows, key=lambda r: r["walk_cycles"])
print(f"# {label}: k_autocorr_wt consumer waves of workgroup 0, {ntiles} hand-overs, "
      f"tiles 1..{ntiles - 1} ({steps} steps each)")
print(f"{'wave':>4s} {'lags':8s} {'walk':>10s} {'/step':>7s} {'tile 0':>9s} {'barrier':>10s} {'/hand-over':>11s} "
      f"{'first wait':>11s} {'later /h-o':>11s}")
for r in rows:
    print(f"{r['wave']:4d} {r['lags']:8s} {r['walk_cycles']:10d} {r['walk_cycles_per_step']:7.2f} "
          f"{r['tile0_cycles']:9d} {r['barrier_cycles']:10d} {r['barrier_cycles_per_handover']:11.1f} "
          f"{r['first_wait_cycles']:11d} {r['later_barrier_cycles_per_handover']:11.1f}")
print(f"slowest walk: wave {slow['wave']} {slow['lags']}")
out = {"label": label, "tile": tile, "handovers": ntiles, "waves": rows, "slowest": slow["wave"]}
# the producers' slots live in K1's own stamp array (k1_autocorr.hip: ACCUM_P, STAMP_HWID)
if k1 is not None:
    sk = st
    passes = n // 128
    simd = [(sk[16 + w] >> 4) & 3 for w in range(8)]
    prods = []
    for q in range(4):
        stage, issue, bar = sk[q], sk[4 + q], sk[8 + q]
        prods.append({"wave": 4 + q, "rows": split[q], "simd": simd[4 + q], "staging_cycles": stage,
                      "issue_loads_cycles": issue, "barrier_cycles": bar,
                      "staging_cycles_per_row_pass": round(stage / (passes * split[q]), 1),
                      "staging_cycles_per_tile": round(stage / ntiles, 1),
                      "barrier_cycles_per_handover": round(bar / ntiles, 1)})
    print(f"# producer waves (rows {split}), {passes} passes of 128 positions; SIMD of consumers 0..3: {simd[:4]}")
    print(f"{'wave':>4s} {'rows':>4s} {'simd':>4s} {'staging':>10s} {'/row-pass':>10s} {'/tile':>9s} {'issue loads':>12s} "
          f"{'barrier':>10s} {'/hand-over':>11s}")
    for r in prods:
        print(f"{r['wave']:4d} {r['rows']:4d} {r['simd']:4d} {r['staging_cycles']:10d} "
              f"{r['staging_cycles_per_row_pass']:10.1f} {r['staging_cycles_per_tile']:9.1f} "
              f"{r['issue_loads_cycles']:12d} {r['barrier_cycles']:10d} {r['barrier_cycles_per_handover']:11.1f}")
    out["producers"] = prods
    out["consumer_simd"] = simd[:4]
print(json.dumps(out))
