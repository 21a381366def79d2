"""Source streams and witnesses for the set layer's tests (DecodeSet, decode_windows of a set, RecodeSet) that do not
depend on the code under test.  Every source stream is made on the CPU: by the oracle's flake_encode_frame() loop
(oracle/flake_oracle.c) or by the pure-Python frame writer (tests/flacgen.py); every expected recode output is the
oracle's loop over the stream's PCM cut at the output block.  tests/test_set_cases_cpu.py holds the inputs and the
witnesses to the independent decoder (oracle/flac_decode.c) and reads each family's built-for property back;
tests/test_gpu_set_matrix.py holds the sets to them.

A stream is a dict like the ones test_gpu_decode_set.encode_set returns: pcm [n][channels] int32 (read-only), frames
(uint8), sizes (int32), off, si_bytes (the 34 STREAMINFO bytes a correct encoder writes for these frames), and md5,
blocks (the frames' sample counts), vbs.  A case is a dict: name, family, ch, bps, streams, B (the recode's output
block), level, flags, batch (FLAKE_AMD_BATCH), calls ([[(stream, first frame, frames)]]: the runs of each call) and
src_max (the largest source block).  Cases are built on first use and shared: nothing in them may be changed.

Families: F1 formats, F2 geometry, F3 long carries, F4 foreign frames, F5 incompressible (see each maker)."""
from __future__ import annotations

import hashlib
import math
import struct
import time

import numpy as np

import flake_amd
import flacgen
import oraclelib
from cases import _rng, full_scale

V = flake_amd
RATE = 44100
VERBATIM, CARRY, DEC = 1, 0, 1            # fo_subframe.type of a VERBATIM subframe; src_buf of a gather piece

TIMES = {}                                # family -> seconds spent generating its cases and expectations
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = oraclelib.Oracle()
    return _oracle


# ---- STREAMINFO and the stream's hash, restated ---------------------------------------------------------------------

def packed_le(pcm, bps):
    """The samples as the stream MD5 reads them: (bps + 7) // 8 bytes each, little-endian, interleaved."""
    nb = (bps + 7) // 8
    return np.ascontiguousarray(np.asarray(pcm).astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def streaminfo34(min_block, max_block, min_frame, max_frame, ch, bps, total, md5, rate=RATE):
    v = (rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | total
    return struct.pack(">HH", min_block, max_block) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + \
        v.to_bytes(8, "big") + md5


def verbatim_size(ch, bps, n):
    """The size above which flake_encode_frame() writes a block again as VERBATIM, and where max_frame_size starts."""
    return 16 + ((n * (2 * bps + 1) + 7) >> 3) if ch == 2 else 16 + ((n * ch * bps + 7) >> 3)


def make_stream(pcm, frames, blocks, ch, bps, vbs):
    pcm = np.ascontiguousarray(pcm, np.int32).reshape(-1, ch)
    assert sum(blocks) == len(pcm) and len(frames) == len(blocks)
    pcm.setflags(write=False)
    sizes = np.array([len(f) for f in frames], np.int32)
    md5 = hashlib.md5(packed_le(pcm, bps)).digest()
    data = np.frombuffer(b"".join(frames), np.uint8)
    return dict(pcm=pcm, frames=data, sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]).astype(int), md5=md5,
                si_bytes=streaminfo34(min(blocks), max(blocks), int(sizes.min()), int(sizes.max()), ch, bps, len(pcm), md5),
                blocks=list(blocks), vbs=bool(vbs))


# ---- the two makers of source streams -------------------------------------------------------------------------------

def oracle_fixed(pcm, ch, bps, n):
    """The oracle's loop over pcm in fixed blocks of n at level 5, the short last frame included."""
    p = V.level_params(5, channels=ch, bits_per_sample=bps, block_size=max(n, 16))
    frames, blocks = [], []
    for j, a in enumerate(range(0, len(pcm), n)):
        blk = pcm[a:a + n]
        rc, out, _, _, _ = oracle().encode_frame(p, j, blk, len(blk))
        assert rc > 0
        frames.append(out.tobytes())
        blocks.append(len(blk))
    return make_stream(pcm, frames, blocks, ch, bps, False)


def vbs_pieces(p, first, blk):
    """One block of a variable-block-size stream through oracle.encode_block, and the frames it became: (bytes, [(size
    in bytes, samples, every subframe VERBATIM)]).  The pieces are split_frame_v1's, encoded one by one; their bytes
    are the block's."""
    n, ch = blk.shape
    rc, out, _ = oracle().encode_block(p, first, blk, n, 8 * n * ch * 4 + 4096)
    assert rc > 0
    psz = [n]
    if n % 8 == 0 and n >= 128:
        nf, sizes = oracle().vbs_split(blk, ch, n)
        if nf > 1:
            psz = [int(q) for q in sizes]
    parts, facts, at = [], [], 0
    for q in psz:
        r2, o2, sf, _, _ = oracle().encode_frame(p, first + at, blk[at:at + q], q)
        assert r2 > 0
        parts.append(o2.tobytes())
        facts.append((r2, q, bool(np.all(sf["type"] == VERBATIM))))
        at += q
    assert b"".join(parts) == out.tobytes()
    return parts, facts


def oracle_vbs(pcm, ch, bps, cuts):
    """A variable-block-size stream (frames numbered by their first sample): the oracle's level-10 loop over pcm cut
    into blocks of cuts[0], cuts[1], ... samples."""
    assert sum(cuts) == len(pcm)
    p = V.level_params(10, channels=ch, bits_per_sample=bps, block_size=max(max(cuts), 128))
    frames, blocks, at = [], [], 0
    for n in cuts:
        parts, facts = vbs_pieces(p, at, pcm[at:at + n])
        frames += parts
        blocks += [q for _, q, _ in facts]
        at += n
    return make_stream(pcm, frames, blocks, ch, bps, True)


def foreign_stream(n, nch, ch_code, bps, vbs, nframes, first, tail, seed):
    """Frames this project's encoder never writes: test_gpu_decode_windows.gen_stream's loop (flacgen.frame over
    gen_specs' rotation of subframe forms), which here keeps the PCM it wrote and the forms it wrote them in.  The
    rotation has FIXED orders 1 to 4; every third frame's last subframe is the catalogue's FIXED order 0."""
    from test_gpu_decode_windows import gen_specs
    frames, parts, blocks, forms = [], [], [n] * nframes + ([tail] if tail else []), set()
    number = first
    for k, m in enumerate(blocks):
        specs = gen_specs(m, nch, k, bps)
        if k % 3 == 1:
            specs[-1] = dict(kind="fixed", order=0, porder=2)
        stereo = ch_code is not None and ch_code >= 8
        if stereo:                       # (the subframes are not the channels: keep to forms any values take)
            specs = [sp if sp["kind"] != "constant" and not sp.get("wasted") else dict(kind="fixed", order=2, porder=1) for sp in specs]
        if m < 16 or m % 4:              # (partitions divide the block and hold at least the predictor's order)
            specs = [dict(sp, porder=0, escape=()) if sp["kind"] in ("fixed", "lpc") else sp for sp in specs]
        pcm = flacgen.test_signal(m, nch, bps, seed=seed + 10 * k + nch)
        for c, sp in enumerate(specs):
            if stereo:
                continue
            if sp["kind"] == "constant":
                pcm[:, c] = -5 - c
            elif sp.get("wasted"):
                pcm[:, c] = (pcm[:, c] >> sp["wasted"]) << sp["wasted"]
        frames.append(flacgen.frame(pcm, number, bps, RATE, specs, ch_code=ch_code, vbs=vbs))
        forms |= {(sp["kind"], sp.get("order", 0), sp.get("method", 0), sp.get("wasted", 0), bool(sp.get("escape"))) for sp in specs}
        parts.append(pcm)
        number += m if vbs else 1
    x = make_stream(np.concatenate(parts), frames, blocks, nch, bps, vbs)
    x["forms"] = sorted(forms)          # (kind, order, Rice method, wasted bits, escapes) as handed to flacgen.frame
    return x


# ---- signals --------------------------------------------------------------------------------------------------------

def resonator(n, ch, bps, seed):
    return V.synth_pcm(1, n, ch, bps, first_frame=seed).reshape(n, ch)


def white(r, n, ch, bps):
    """cases.fuzz_signal's kind 1 at shift 0: full-scale white noise."""
    full = 1 << (bps - 1)
    return r.randint(-full, full, (n, ch)).astype(np.int32)


def loud_white(r, n, ch, bps):
    """White noise kept to the outer half of the range: a Rice code takes bps + 1 bits for every sample of it.  For
    stereo, where flake_encode_frame() turns to VERBATIM only above 2 bps + 1 bits a sample pair and plain white noise
    is Rice-coded at about 2 bps + 0.8, just below that."""
    half = 1 << (bps - 2)
    x = white(r, n, ch, bps).astype(np.int64)
    return np.where(x >= 0, np.maximum(x, x ^ half), np.minimum(x, x ^ half)).astype(np.int32)


def random_full_scale(r, n, ch, bps):
    """cases.edge_blocks' alt_full_scale (+max and -min only) with the sign drawn per sample: the plain alternation has
    x[i] + x[i-1] = -1, which an LPC of order 1 predicts exactly, so it compresses and is not what F5 is for."""
    fs = full_scale(bps)
    return np.where(r.randint(0, 2, (n, ch)) == 1, fs, -fs - 1).astype(np.int32)


def mixed_full_scale(r, n, ch, bps, e):
    """Runs of e samples in turn: white noise (stereo: loud_white) in every channel, then random full scale in the even
    channels beside that noise in the odd ones (random full scale in both channels of a stereo pair leaves a side channel that is zero half
    of the time, and compresses).  Both are incompressible, and their second differences differ enough for
    split_frame_v1 to cut a block at every change."""
    pick = ((np.arange(n) // max(e, 1)) % 2 == 0)[:, None] & (np.arange(ch) % 2 == 0)[None, :]
    return np.where(pick, random_full_scale(r, n, ch, bps), (loud_white if ch == 2 else white)(r, n, ch, bps)).astype(np.int32)


# ---- the expected output of a recode --------------------------------------------------------------------------------

def encoder_params(ch, bps, B, level):
    """What StreamSet(level=level, block_size=B, channels=ch, bits_per_sample=bps) encodes with."""
    return V.level_params(level, channels=ch, bits_per_sample=bps, block_size=B)


def expected_stream(pcm, ch, bps, B, level, vbs):
    """The oracle's loop over pcm cut at B: dict(whole: the bytes of the whole blocks, all: with the tail, si: the 34
    STREAMINFO bytes, frames: [(bytes, samples, all VERBATIM)] of every frame, block_bytes: per block)."""
    p = encoder_params(ch, bps, B, level)
    assert bool(p.variable_block_size) == bool(vbs)
    nb = len(pcm) // B
    cuts = [(j * B, B) for j in range(nb)] + ([(nb * B, len(pcm) - nb * B)] if len(pcm) % B else [])
    data, facts, block_bytes = [], [], []
    for j, (a, n) in enumerate(cuts):
        blk = pcm[a:a + n]
        if vbs:
            parts, f = vbs_pieces(p, a, blk)
            data.append(b"".join(parts))
            facts += f
        else:
            rc, out, sf, _, _ = oracle().encode_frame(p, j, blk, n)
            assert rc > 0
            data.append(out.tobytes())
            facts.append((rc, n, bool(np.all(sf["type"] == VERBATIM))))
        block_bytes.append(len(data[-1]))
    md5 = hashlib.md5(packed_le(pcm, bps)).digest()
    largest = max([f[0] for f in facts] + [verbatim_size(ch, bps, B)])
    return dict(whole=b"".join(data[:nb]), all=b"".join(data), frames=facts, block_bytes=block_bytes, md5=md5,
                si=streaminfo34(16 if vbs else B, B, 0, largest, ch, bps, len(pcm), md5))


_expected = {}


def expected(case):
    """expected_stream of every stream of the case as its calls feed it, made once."""
    if case["name"] not in _expected:
        t0 = time.perf_counter()
        # (a stream that no call names stays empty)
        _expected[case["name"]] = [expected_stream(x["pcm"] if s in case["named"] else x["pcm"][:0], case["ch"], case["bps"],
                                                   case["B"], case["level"], bool(case["flags"] & V.SET_VBS))
                                   for s, x in enumerate(case["streams"])]
        TIMES[case["family"]] = TIMES.get(case["family"], 0.0) + time.perf_counter() - t0
    return _expected[case["name"]]


# ---- runs and calls -------------------------------------------------------------------------------------------------

def round_robin(streams, per, named):
    """[(stream, first frame, frames)]: `per` frames of every named stream in turn until all are used up."""
    at = {s: 0 for s in named}
    runs = []
    while any(at[s] < len(streams[s]["sizes"]) for s in named):
        for s in named:
            n = min(per, len(streams[s]["sizes"]) - at[s])
            if n > 0:
                runs.append((s, at[s], n))
                at[s] += n
    return runs


def dealt(streams, r, max_run, absent=None, lead=None):
    """Runs dealt out irregularly: a stream and 1 .. max_run of its next frames, drawn from r, until all are used up.
    absent = (stream, from, to): that stream gets nothing while the frames dealt so far are in [from, to).  lead: the
    stream whose first frame is the first run."""
    at = [0] * len(streams)
    runs, done = [], 0
    if lead is not None:
        runs, done = [(lead, 0, 1)], 1
        at[lead] = 1
    while True:
        live = [s for s in range(len(streams)) if at[s] < len(streams[s]["sizes"])]
        if not live:
            return runs
        pick = [s for s in live if not (absent and s == absent[0] and absent[1] <= done < absent[2])] or live
        s = pick[int(r.randint(0, len(pick)))]
        n = min(int(r.randint(1, max_run + 1)), len(streams[s]["sizes"]) - at[s])
        runs.append((s, at[s], n))
        at[s] += n
        done += n


def in_calls(runs, per_call):
    return [runs[i:i + per_call] for i in range(0, len(runs), per_call)]


def as_call(streams, runs, frames=None):
    """The runs as DecodeSet.decode_runs and RecodeSet.recode_runs take them."""
    return [(s, (frames[s] if frames else streams[s]["frames"])[streams[s]["off"][a]:streams[s]["off"][a + n]],
             streams[s]["sizes"][a:a + n]) for s, a, n in runs]


def like_of(case):
    return V.HostStreaminfo(min_block_size=16, max_block_size=case["src_max"], sample_rate=RATE, channels=case["ch"],
                            bits_per_sample=case["bps"])


def steps_of(case):
    """The decode batches ("steps") the case's calls make, as decode_set_plan.h cuts them: each call's frames back to
    back, at most `batch` a step, the part of a run inside a step one segment.  [(segments [(stream, start, samples)],
    the frames' starts)], both counted in samples from the step's first."""
    steps = []
    for call in case["calls"]:
        frames = [(s, case["streams"][s]["blocks"][a + i], r) for r, (s, a, n) in enumerate(call) for i in range(n)]
        for f0 in range(0, len(frames), case["batch"]):
            segs, starts, at = [], [], 0
            for s, m, r in frames[f0:f0 + case["batch"]]:
                if segs and segs[-1][3] == r:
                    segs[-1][2] += m
                else:
                    segs.append([s, at, m, r])
                starts.append(at)
                at += m
            steps.append(([(s, start, m) for s, start, m, _ in segs], starts))
    return steps


def want_decode_batches(case):
    return sum(math.ceil(sum(n for _, _, n in call) / case["batch"]) for call in case["calls"])


# ---- the families ---------------------------------------------------------------------------------------------------

F1_PAIRS = [(1, 8), (1, 16), (2, 12), (2, 24), (3, 24), (6, 20), (8, 32), (2, 32)]
F1_B, F1_SRC = 576, 192
F2_PAIRS = [(2, 16), (3, 24)]
F2_GEOM = [(1152, 4096), (4608, 4096), (4096, 1152), (4096, 4096)]
F5_PAIRS = [(2, 16), (2, 24), (1, 8), (8, 24)]
F5_OUT = [(16, 5), (192, 5), (4096, 5), (4096, 10)]


def _case(name, family, ch, bps, streams, B, level, flags, batch, calls):
    return dict(name=name, family=family, ch=ch, bps=bps, streams=streams, B=B, level=level, flags=flags, batch=batch,
                calls=calls, src_max=max(max(x["blocks"]) for x in streams),
                named=sorted({s for call in calls for s, _, _ in call}))


def f1(ch, bps):
    """Formats.  Source block 192; five streams: one sample, B - 1, exactly 2 B, 2 B + 1 (its last frame is one
    sample), and one that is in the set and never named.  B = 576 = 3 source frames, so that the named streams are 1,
    3, 6 and 7 frames: 17 frames, three device batches of 7."""
    lens = [1, F1_B - 1, 2 * F1_B, 2 * F1_B + 1, 100]
    streams = [oracle_fixed(resonator(n, ch, bps, 300 + 10 * ch + s), ch, bps, F1_SRC) for s, n in enumerate(lens)]
    calls = in_calls(round_robin(streams, 3, [0, 1, 2, 3]), 3)
    c = _case(f"F1-{ch}x{bps}", "F1", ch, bps, streams, F1_B, 5, 0, 7, calls)
    c["lens"] = lens
    return c


def f2(ch, bps, src, B):
    """Geometry.  Four streams of 3 to 4 blocks of the larger of the two sizes plus a tail, so that every stream has
    several whole source frames and several whole output blocks; stream 1 has variable block size and a first frame
    of 1151 samples, so that every later sample of it disagrees with its destination modulo 16 bytes."""
    r = _rng(2000 + src + B + ch)
    tails = [17, 333, 1000, 8]
    streams = []
    for s in range(4):
        n = (3 + s % 2) * max(src, B) + tails[s]
        pcm = resonator(n, ch, bps, 400 + s + ch) if s != 2 else np.ascontiguousarray(
            (white(r, n, ch, bps).astype(np.int64) >> 3).astype(np.int32))
        if s == 1:
            cuts = [1151] + [src] * ((n - 1151) // src)
            cuts += [n - sum(cuts)] if n - sum(cuts) else []
            streams.append(oracle_vbs(pcm, ch, bps, cuts))
        else:
            streams.append(oracle_fixed(pcm, ch, bps, src))
    calls = in_calls(round_robin(streams, 3, [0, 1, 2, 3]), 4)
    return _case(f"F2-{ch}x{bps}-{src}to{B}", "F2", ch, bps, streams, B, 5, 0, 5, calls)


def f3(nstreams):
    """Long carries, stereo 16 bit, source block 16.  Three streams to output block 2048: 7 frames a step are 112
    samples, so a stream that got every frame would wait 18 steps for its first block; the runs are dealt out
    irregularly and stream 2 gets nothing while frames 200 .. 320 are dealt (17 steps) although it holds a carry.
    Seventy streams to output block 64: more streams than one wave has lanes, and ten device batches of tails; stream 11
    gets the first frame of all and then nothing while frames 1 .. 120 are dealt (17 steps)."""
    r = _rng(3000 + nstreams)
    if nstreams == 3:
        lens, B, absent, max_run, lead = [4200, 2300, 2100], 2048, (2, 200, 320), 5, None
    else:
        lens = [64 * int(r.randint(1, 3)) + (0 if s % 23 == 5 else int(r.randint(1, 64))) for s in range(nstreams)]
        B, absent, max_run, lead = 64, (11, 1, 120), 4, 11
    streams = [oracle_fixed(resonator(n, 2, 16, 500 + s), 2, 16, 16) for s, n in enumerate(lens)]
    calls = in_calls(dealt(streams, r, max_run, absent, lead), 40)
    c = _case(f"F3-{nstreams}", "F3", 2, 16, streams, B, 5, 0, 7, calls)
    c["absent"] = absent[0]
    return c


F4_SETS = {
    # name: (channels, bits, output block, [(block, channel assignment, variable, frames, first number, tail)])
    "1x16": (1, 16, 96, [(192, None, False, 5, 0, 50), (192, None, True, 4, 0, 7), (16, None, False, 9, 3, 0)]),
    "2x16": (2, 16, 96, [(192, 1, False, 5, 0, 100), (192, 8, True, 4, 0, 0), (192, 9, False, 4, 3, 31), (192, 10, True, 6, 0, 5)]),
    "2x24": (2, 24, 4096, [(1152, 10, False, 4, 0, 100), (1152, 8, True, 4, 0, 0), (1152, 1, False, 5, 0, 9)]),
    "3x24": (3, 24, 96, [(192, None, False, 5, 0, 60), (192, None, True, 4, 0, 0), (16, None, True, 8, 0, 5)]),
}


def f4(name):
    """Foreign frames: independent, left/side, right/side and mid/side stereo, wasted bits, CONSTANT, VERBATIM, FIXED
    0 .. 4 and LPC subframes, both Rice methods, escapes, fixed and variable blocking, a first number that is not 0."""
    ch, bps, B, rows = F4_SETS[name]
    streams = [foreign_stream(n, ch, cc, bps, vbs, nf, first, tail, 4000 + 100 * i + n)
               for i, (n, cc, vbs, nf, first, tail) in enumerate(rows)]
    calls = in_calls(round_robin(streams, 3, list(range(len(streams)))), 3)
    return _case(f"F4-{name}", "F4", ch, bps, streams, B, 5, 0, 7, calls)


def f5(ch, bps, B, level):
    """Incompressible.  Stream 0 is full-scale white noise (stereo: loud_white) in whole source frames that are whole output blocks, alone
    in the first call: that call's bound (flake_amd_recode_set_out_bound) counts exactly the blocks it writes, all of
    them VERBATIM.  Stream 1 (mixed_full_scale) changes every eighth of an output block, so that at level 10 the splitter
    cuts it into eight frames, and has a tail.  Source block 1152 (4096 for output block 4096)."""
    r = _rng(5000 + 100 * ch + bps + B + level)
    src = 4096 if B == 4096 else 1152
    n0 = 2 * 4096 if B == 4096 else 1152
    n1 = 4096 + 1000 if B == 4096 else 2 * B + B // 2 + 3
    streams = [oracle_fixed((loud_white if ch == 2 else white)(r, n0, ch, bps), ch, bps, src), oracle_fixed(mixed_full_scale(r, n1, ch, bps, B // 8), ch, bps, src)]
    calls = [[(0, 0, len(streams[0]["sizes"]))], [(1, 0, len(streams[1]["sizes"]))]]
    return _case(f"F5-{ch}x{bps}-b{B}-l{level}", "F5", ch, bps, streams, B, level, V.SET_VBS if level >= 9 else 0, 7, calls)


_MAKERS = {}
for _ch, _bps in F1_PAIRS:
    _MAKERS[f"F1-{_ch}x{_bps}"] = (f1, (_ch, _bps))
for _ch, _bps in F2_PAIRS:
    for _src, _B in F2_GEOM:
        _MAKERS[f"F2-{_ch}x{_bps}-{_src}to{_B}"] = (f2, (_ch, _bps, _src, _B))
for _n in (3, 70):
    _MAKERS[f"F3-{_n}"] = (f3, (_n,))
for _name in F4_SETS:
    _MAKERS[f"F4-{_name}"] = (f4, (_name,))
for _ch, _bps in F5_PAIRS:
    for _B, _level in F5_OUT:
        _MAKERS[f"F5-{_ch}x{_bps}-b{_B}-l{_level}"] = (f5, (_ch, _bps, _B, _level))

NAMES = sorted(_MAKERS)
_cases = {}


def names(*families):
    return [n for n in NAMES if n[:2] in families]


def case(name):
    if name not in _cases:
        fn, args = _MAKERS[name]
        t0 = time.perf_counter()
        _cases[name] = fn(*args)
        assert _cases[name]["name"] == name
        TIMES[name[:2]] = TIMES.get(name[:2], 0.0) + time.perf_counter() - t0
    return _cases[name]
