"""Inputs shared by the ragged variable-block-size tests (test_gpu_vbs_ragged_abi.py, test_gpu_set_vbs_ragged.py): blocks
of different lengths on handles with block_size 1152 (an eighth of 144), the signal bursts against near-silence per
eighth (the idea of burst_block in test_gpu_set_vbs.py) so that split_frame_v1 cuts a good part of the blocks it sees.
Not a test module: nothing here is collected."""
import numpy as np

BS = 1152

# lengths split_frame_v1 sees (a multiple of 8, at least 128: encode.c:997-999) and lengths that are one frame
SPLIT_LOW = [1152, 1144, 1000, 640, 512, 264, 136, 128]
ONE_LOW = [1151, 333, 257, 120, 104, 77, 17]
# levels 11 / 12 search up to order 32: every piece holds at least 64 samples
SPLIT_HIGH = [1152, 1144, 1024, 1000, 640, 520, 512]
ONE_HIGH = [1151, 333, 257, 120, 104, 77, 65]


def splittable(n):
    return n % 8 == 0 and n >= 128


def lengths_for(level):
    """The blocks of a case in call order: splittable and one-frame lengths alternate, the odd lengths in front, so that
    the splittable blocks start at every offset modulo 4 samples (mono: bytes 0, 4, 8, 12 modulo 16; stereo: 0 and 8;
    three channels: a non-multiple of 8)."""
    sp, one = (SPLIT_HIGH, ONE_HIGH) if level >= 11 else (SPLIT_LOW, ONE_LOW)
    out = []
    for i in range(max(len(sp), len(one))):
        if i < len(sp):
            out.append(sp[i])
        if i < len(one):
            out.append(one[i])
    return out


def burst_block(r, n, ch, bits, kind):
    """One block of n samples: every eighth is a noise burst or near-silence.  kind 0: all eighths loud alike (the
    splitter leaves such a block whole); 1: a random pattern with at least one change; 2: loud, quiet, quiet, then loud
    -- cuts behind the first and the third eighth: three frames of unequal lengths."""
    # (no louder than 16-bit audio: the reference scales a score difference by 200 in 32 bits, vbs.c:69, and louder
    # bursts wrap there -- cuts then fall anywhere)
    loud, quiet = 1 << (min(bits, 16) - 3), 3
    e = max(n // 8, 1)
    pat = np.ones(8, np.int64)
    if kind == 2:
        pat = np.array([1, 0, 0, 1, 1, 1, 1, 1])
    elif kind:
        while pat.min() == pat.max():
            pat = r.randint(0, 2, 8)
    amp = np.where(np.repeat(pat, e)[:n] > 0, loud, quiet) if n >= 8 else np.full(n, loud)
    amp = np.concatenate([amp, np.full(n - len(amp), amp[-1] if len(amp) else loud)])
    base = (r.uniform(-1.0, 1.0, n) * amp).astype(np.int64)
    out = np.empty((n, ch), np.int32)
    for c in range(ch):
        out[:, c] = base + (r.uniform(-1.0, 1.0, n) * np.maximum(amp // 16, 1)).astype(np.int64)
    lim = (1 << (bits - 1)) - 1
    return np.clip(out, -lim - 1, lim)


def make_blocks(seed, lengths, ch, bits):
    """One block per length; of the splittable ones the first stays whole, the second becomes three frames, the others
    follow a random pattern."""
    r = np.random.RandomState(seed)
    blocks, k = [], 0
    for n in lengths:
        kind = 1
        if splittable(n):
            kind = (0, 2)[k] if k < 2 else 1
            k += 1
        blocks.append(burst_block(r, n, ch, bits, kind))
    return blocks


def oracle_splits(oracle, blocks, ch):
    """split_frame_v1 on the CPU per splittable block, (1, [n]) for the others; asserts that the case is worth running:
    of the splittable blocks at least one stays whole, at least a third are cut, and at least one becomes three or more
    frames of unequal lengths."""
    res = []
    for b in blocks:
        n = b.shape[0]
        if splittable(n):
            nf, sizes = oracle.vbs_split(b, ch, n)
            res.append((int(nf), [int(x) for x in sizes]))
        else:
            res.append((1, [n]))
    sp = [res[i] for i, b in enumerate(blocks) if splittable(b.shape[0])]
    assert any(nf == 1 for nf, _ in sp), sp
    assert 3 * sum(1 for nf, _ in sp if nf > 1) >= len(sp), sp
    assert any(nf >= 3 and len(set(sizes)) > 1 for nf, sizes in sp), sp
    return res


def byte_offsets(lengths, ch):
    """Byte offset of every block in the back-to-back int32 PCM."""
    return [4 * ch * int(x) for x in np.concatenate([[0], np.cumsum(lengths)[:-1]])]
