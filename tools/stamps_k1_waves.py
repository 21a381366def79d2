"""Diagnostic (not part of the product): walk cycles of each of the four consumer waves of
k_autocorr_wt's workgroup 0 at the headline (configs[1]: 4096 stereo frames, n = 4096, LPC-8).
The tile time is set by the slowest walk; the other waves wait for it at the next barrier.
The tile is 256 positions (128 steps per parity) in the long-tile form and 128 (64 steps) in the 128 form
(FHIP_WT_TILE=128 in the environment keeps the latter): fhip_autocorr_tile says which ran.
Needs the stamped build (add -DFHIP_PROBE_NOB for the probe that drops every b0 read):
  python -c "from flake_amd.build import build_hip; build_hip(True, ['-DFHIP_STAMPS'], 'libflakehip_dbg.so')"
  FHIP_LIB=flake_amd/lib/libflakehip_dbg.so python tools/stamps_k1_waves.py [label]"""
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
fa.load_library().fhip_debug_read_stamps(st)
groups = ["{0,2,4}", "{6,8}", "{1,3}", "{5,7}"]            # launch_autocorr's split at max order 8
lib = fa.load_library()
tile = lib.fhip_autocorr_tile(nfr * 2, n, 8) if hasattr(lib, "fhip_autocorr_tile") else 128   # (older builds: 128)
ntiles, steps = n // tile, tile // 2
rows = []
for w in range(4):
    walk, t0, bar = st[48 + w], st[52 + w], st[56 + w]
    rows.append({"wave": w, "lags": groups[w], "walk_cycles": walk, "tile0_cycles": t0, "barrier_cycles": bar,
                 "walk_cycles_per_step": round(walk / ((ntiles - 1) * steps), 2),
                 "barrier_cycles_per_handover": round(bar / ntiles, 1)})
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.environ.get("FHIP_LIB", "libflakehip.so"))
slow = max(rows, key=lambda r: r["walk_cycles"])
print(f"# {label}: k_autocorr_wt consumer waves of workgroup 0, {ntiles} hand-overs, "
      f"tiles 1..{ntiles - 1} ({steps} steps each)")
print(f"{'wave':>4s} {'lags':8s} {'walk':>10s} {'/step':>7s} {'tile 0':>9s} {'barrier':>10s} {'/hand-over':>11s}")
for r in rows:
    print(f"{r['wave']:4d} {r['lags']:8s} {r['walk_cycles']:10d} {r['walk_cycles_per_step']:7.2f} "
          f"{r['tile0_cycles']:9d} {r['barrier_cycles']:10d} {r['barrier_cycles_per_handover']:11.1f}")
print(f"slowest walk: wave {slow['wave']} {slow['lags']}")
print(json.dumps({"label": label, "tile": tile, "handovers": ntiles, "waves": rows, "slowest": slow["wave"]}))
