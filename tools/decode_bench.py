"""Cost of K7 (the on-device decoder) against its neighbours, written to profiles/decode_bench.txt.

    python tools/decode_bench.py [--reps R] [--out FILE]

Two batches: the headline one (4096 stereo 16-bit frames of 4096 samples, level 5) and a level-12 batch of 1024
blocks of 8192 (variable block size: the frames the encoder cut them into).  Per batch, four figures:

  k_decode   K7's three launches, hipEvents around them (fhip_get_kernel_times), fhip_decode_frames_dev on a
             device-resident stream
  host       flake_amd_decode_frames on the same frames from host memory: upload, K7, download, the MD5
  k_verify   K5 on the same stream and its PCM (fhip_verify_frames_dev), the same way: K5's code is the parent's
  cpu        oracle/flac_decode.c (the test decoder, built as oracle/libflac_decode.so) on one core, over the first
             frames of the batch, scaled to the batch by samples
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import flake_amd  # noqa: E402
import oraclelib  # noqa: E402

P = flake_amd.level_params


def encode_fixed(enc, pcm, n):
    import ctypes as C
    nf = pcm.shape[0]
    fb = np.zeros(nf, np.int32)
    b = flake_amd.Batch()
    b.pcm, b.nframes, b.block_size, b.frame_bytes = pcm.ctypes.data, nf, n, fb.ctypes.data
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = C.c_int64(0)
    rc = enc.lib.fhip_encode_frames_packed(enc._h, C.byref(b), out.ctypes.data, cap, C.byref(wrote))
    assert rc == 0, enc.lib.fhip_last_error(enc._h)
    return out[:wrote.value].copy(), fb


def encode_vbs(enc, pcm, nb, n, dev):
    dp = torch.from_numpy(pcm.reshape(-1)).to(dev)
    cap = 8 * nb * enc.frame_stride(n)
    dpk = torch.zeros(cap, dtype=torch.uint8, device=dev)
    dfb = torch.zeros(8 * nb, dtype=torch.int32, device=dev)
    dt = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    enc.encode_blocks_vbs_dev(dp, nb, n, dpk, cap, dt, frame_bytes=dfb)
    enc.sync()
    nf, nbytes = int(dt[0]), int(dt[1])
    return dpk.cpu().numpy()[:nbytes].copy(), dfb.cpu().numpy()[:nf].copy()


def bench(name, p, nblocks, vbs, reps, lines):
    n, ch = p.block_size, p.channels
    dev = torch.device("cuda")
    pcm = flake_amd.synth_pcm(nblocks, n, ch, p.bits_per_sample)
    flat = pcm.reshape(-1, ch)
    with flake_amd.Encoder(p, max_frames=nblocks * (8 if vbs else 1)) as enc:
        s, fb = encode_vbs(enc, pcm, nblocks, n, dev) if vbs else encode_fixed(enc, pcm, n)
        nf, total = len(fb), nblocks * n
        ds, dfb = torch.from_numpy(s).to(dev), torch.from_numpy(fb).to(dev)
        dp = torch.from_numpy(flat.reshape(-1)).to(dev)
        dout = torch.zeros(total * ch, dtype=torch.int32, device=dev)
        dsum = torch.zeros(4, dtype=torch.int64, device=dev)
        dns = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        dec = (ds, len(s), dfb, nf, dout, total, dsum, dns, None, vbs, 0)
        ver = (ds, len(s), dfb, nf, dp, total, 0, dsum)
        res = {}
        for what, fn, args in (("k_decode", enc.decode_frames_dev, dec), ("k_verify", enc.verify_frames_dev, ver)):
            fn(*args)                              # first launch: code objects, workspace
            enc.sync()
            assert int(dsum[1]) == 0, (what, dsum)
            enc.set_profiling(True)
            enc.kernel_times(reset=True)
            for _ in range(reps):
                fn(*args)
            enc.sync()
            ms, cnt = enc.kernel_times(reset=True)[what]
            enc.set_profiling(False)
            res[what] = ms / cnt
        assert int(dns[0]) == total and np.array_equal(dout.cpu().numpy().reshape(-1, ch), flat)
    # the host path: its own handle, FLAKE_AMD_BATCH frames per chunk
    si = flake_amd.HostStreaminfo(min_block_size=16 if vbs else n, max_block_size=n, sample_rate=p.sample_rate,
                                  channels=ch, bits_per_sample=p.bits_per_sample)
    ts = []
    for _ in range(3):
        with flake_amd.HostDecoder(si) as d:
            t0 = time.perf_counter()
            out = d.decode_frames(s, fb, total, 2)
            ts.append(time.perf_counter() - t0)
            assert np.array_equal(out, flat.astype(np.int16))
    res["host"] = min(ts[1:]) * 1e3
    # one CPU core of the test decoder over the first frames, scaled by samples
    k = min(nf, 256)
    cut = int(fb[:k].sum())
    cpu = oraclelib.Decoder()
    t0 = time.perf_counter()
    ref, sizes = cpu.decode(s[:cut], ch, p.bits_per_sample, total)
    dt = time.perf_counter() - t0
    assert np.array_equal(ref, flat[:len(ref)])
    res["cpu"] = dt * 1e3 * total / len(ref)
    msamples = total / 1e6
    lines.append(f"{name}: {nf} frames, {total} samples per channel x {ch}, {len(s)} stream bytes")
    for what, note in (("k_decode", "K7 kernels"), ("host", "flake_amd_decode_frames, host memory, int16 out"),
                       ("k_verify", "K5 kernels, same batch"),
                       ("cpu", f"oracle/flac_decode.c, one core, {k} frames scaled")):
        lines.append(f"  {what:9s} {res[what]:10.3f} ms  {msamples / res[what] * 1e3:10.1f} Msamples/s  ({note})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_bench.txt"))
    a = ap.parse_args()
    lines = ["tools/decode_bench.py: K7 (decode) against K5 (verify), the host path and one CPU core of the test decoder",
             f"device: {torch.cuda.get_device_name(0)}; kernel figures are means of {a.reps} runs, Msamples/s per channel", ""]
    bench("level 5, 4096 blocks of 4096", P(5), 4096, False, a.reps, lines)
    lines.append("")
    bench("level 12, 1024 blocks of 8192", P(12), 1024, True, a.reps, lines)
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
