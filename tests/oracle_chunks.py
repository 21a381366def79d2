"""The CPU oracle over benchmark-size batches: frame chunks (or VBS blocks) on a thread pool, each
chunk compared with the GPU's outputs as soon as it is done, so that host memory stays bounded
(configs[3]'s Rice sections alone are ~800 MB at 4096 frames).  ctypes releases the GIL around the
oracle's calls; chunks are independent (an oracle batch is a loop over frames, a VBS stream a loop
over blocks whose frame numbers count from the stream's start)."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from parity import SCALARS

CHUNK_BYTES = 48 << 20           # oracle output per chunk in flight (x threads: well under 2 GB)


def threads() -> int:
    """Worker threads: the CPUs this process may run on, at most 16 (never os.cpu_count(), which
    counts the whole machine)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _chunks(total, per):
    return [(a, min(total, a + per)) for a in range(0, total, per)]


def _first_failure(jobs):
    """Run the jobs on the pool; re-raise the failure of the earliest chunk (all chunks run)."""
    with ThreadPoolExecutor(threads()) as pool:
        futs = [pool.submit(j) for j in jobs]
        errs = [f.exception() for f in futs]
    for e in errs:
        if e is not None:
            raise e


def info_mismatch(got, exp, s0=0):
    """None, or a message naming the first subframe whose record differs from the oracle's in a
    field the stream carries: the scalars, coefs[:order] (LPC), warmup[:order] (1 for CONSTANT),
    rparams[:1 << porder] (FIXED / LPC)."""
    assert got.shape == exp.shape, (got.shape, exp.shape)
    for k in SCALARS:
        bad = np.nonzero(got[k] != exp[k])[0]
        if bad.size:
            s = int(bad[0])
            return (f"field {k!r} differs in {bad.size}/{got.size} subframes; first subframe {s0 + s}: "
                    f"got {got[k][s]} expected {exp[k][s]}")
    typ, order, porder = exp["type"], exp["order"].astype(np.int64), exp["porder"].astype(np.int64)
    j32 = np.arange(32)[None, :]
    masks = {
        "coefs": (typ == 32)[:, None] & (j32 < order[:, None]),
        "warmup": j32 < np.where(typ == 0, 1, order)[:, None],
        "rparams": ((typ == 8) | (typ == 32))[:, None] & (np.arange(256)[None, :] < (1 << porder)[:, None]),
    }
    for k, m in masks.items():
        bad = np.nonzero(((got[k] != exp[k]) & m).any(axis=1))[0]
        if bad.size:
            s = int(bad[0])
            return f"{k} differ in {bad.size} subframes; first subframe {s0 + s}: got {got[k][s]} expected {exp[k][s]}"
    return None


def residual_mismatch(got, exp, info, s0=0):
    """got / exp [nsub][n]; a CONSTANT subframe defines only residual[0] (optimize.c:147)."""
    diff = got != exp
    diff[info["type"] == 0, 1:] = False
    bad = np.nonzero(diff.any(axis=1))[0]
    if bad.size:
        s = int(bad[0])
        i = int(np.nonzero(diff[s])[0][0])
        return (f"residual differs in {bad.size} subframes; first subframe {s0 + s} at i={i}: "
                f"got {got[s, i]} expected {exp[s, i]}")
    return None


def bits_mismatch(got, exp, info, s0=0):
    """Residual sections byte for byte up to their bit length (got / exp [nsub][>= section bytes])."""
    nbytes = (np.maximum(info["rice_nbits"].astype(np.int64), 0) + 7) // 8
    w = min(got.shape[1], exp.shape[1])
    if nbytes.size and nbytes.max() > w:
        return f"a section of {int(nbytes.max())} bytes does not fit the {w} compared"
    diff = (got[:, :w] != exp[:, :w]) & (np.arange(w)[None, :] < nbytes[:, None])
    bad = np.nonzero(diff.any(axis=1))[0]
    if bad.size:
        s = int(bad[0])
        b = int(np.nonzero(diff[s])[0][0])
        return (f"rice bits differ in {bad.size} subframes; first subframe {s0 + s}, byte {b} of {int(nbytes[s])}: "
                f"got {got[s, b]:#x} expected {exp[s, b]:#x}")
    return None


def compare_batch(oracle, p, pcm, n, info, rice_bits, slot, residual=None, what=""):
    """The oracle's encode_subframes_batch over pcm [nframes][n][ch] against the GPU's outputs of the
    same batch: every record field, every residual section byte and, where given, the residual.
    info: host INFO_DTYPE[nsub]; rice_bits: [nsub][slot] rows (numpy, or a device tensor whose rows
    are fetched a chunk at a time); residual: [nframes][ch][n] host, or None."""
    ch = p.channels
    nframes = pcm.shape[0]
    assert info.shape == (nframes * ch,), (what, info.shape)
    per_frame = ch * (slot + info.dtype.itemsize + (4 * n if residual is not None else 0)) + 4 * n * ch
    per = max(1, min(CHUNK_BYTES // per_frame, -(-nframes // (4 * threads()))))

    def job(f0, f1):
        def run():
            s0, s1 = f0 * ch, f1 * ch
            exp = oracle.encode_subframes_batch(p, pcm[f0:f1], n, want_residual=residual is not None,
                                                slot_bytes=slot)
            msg = info_mismatch(info[s0:s1], exp["info"], s0)
            if msg is None and residual is not None:
                msg = residual_mismatch(residual[f0:f1].reshape(-1, n), exp["residual"].reshape(-1, n),
                                        exp["info"], s0)
            if msg is None:
                w = int((np.maximum(exp["info"]["rice_nbits"].astype(np.int64), 0).max(initial=0) + 7) // 8)
                w = max(4, min(slot, (w + 3) & ~3))
                rows = rice_bits[s0:s1, :w]
                if not isinstance(rows, np.ndarray):
                    rows = rows.cpu().numpy()
                msg = bits_mismatch(rows, exp["rice_bits"][:, :w], exp["info"], s0)
            if msg is not None:
                raise AssertionError(f"{what}: frames {f0}..{f1}: {msg}")
        return run

    _first_failure([job(a, b) for a, b in _chunks(nframes, per)])


def oracle_blocks(oracle, p, blocks, n, first=0, blocks_per_chunk=None):
    """What the flake_encode_frame() loop writes for consecutive blocks [nblocks][n][ch] of one stream
    whose first sample (allow_vbs: frame numbers count samples) or first frame is `first`: the
    stream's bytes and every block's byte count.  Block b's frame counter starts at first + b * n
    (allow_vbs) or first + b."""
    ch = p.channels
    nblocks = blocks.shape[0]
    step = n if p.allow_vbs else 1
    per = blocks_per_chunk or max(1, -(-nblocks // (4 * threads())))
    cap = 8 * n * ch * 4 + 4096
    parts = _chunks(nblocks, per)
    out = [None] * len(parts)

    def job(i, b0, b1):
        def run():
            data, sizes = [], []
            for b in range(b0, b1):
                rc, d, _ = oracle.encode_block(p, first + b * step, blocks[b], n, cap)
                if rc <= 0:
                    raise RuntimeError(f"oracle encode_block failed on block {b}")
                data.append(d)
                sizes.append(rc)
            out[i] = (np.concatenate(data), sizes)
        return run

    _first_failure([job(i, a, b) for i, (a, b) in enumerate(parts)])
    return np.concatenate([o[0] for o in out]), np.array([s for o in out for s in o[1]], dtype=np.int64)


def stream_mismatch(got, exp, got_sizes, exp_sizes):
    """None, or where a packed stream and its block sizes first differ from the oracle's."""
    got_sizes = np.asarray(got_sizes, dtype=np.int64)
    if got_sizes.shape != exp_sizes.shape or (got_sizes != exp_sizes).any():
        bad = np.nonzero(got_sizes[:exp_sizes.size] != exp_sizes[:got_sizes.size])[0]
        b = int(bad[0]) if bad.size else min(got_sizes.size, exp_sizes.size)
        return f"block sizes differ (first block {b}; {got_sizes.size} vs {exp_sizes.size} blocks)"
    if got.size != exp.size:
        return f"stream is {got.size} bytes, the oracle's {exp.size}"
    bad = np.nonzero(got != exp)[0]
    if bad.size:
        ends = np.cumsum(exp_sizes)
        return f"stream differs at {bad.size} bytes; first byte {int(bad[0])} (block {int(np.searchsorted(ends, bad[0], 'right'))})"
    return None
