"""The inputs and witnesses of tests/test_gpu_set_matrix.py (tests/setcases.py) hold on their own, without a device:
every source stream decodes to its PCM with the independent decoder (oracle/flac_decode.c) and is indexed alike by
flake_amd_index_frames (CPU only); every expected recode output decodes back to the same PCM; and what each family was
built for is read back from the inputs, not assumed.  The planner of a recode set (recode_plan.h, through
tools/recode_plan_dump.c as tests/test_recode_plan_cpu.py builds it) is walked over the F2 and F3 segment lists and held
to a restatement in numpy: each stream's carry and segments put together and cut at multiples of the block."""
import numpy as np
import pytest

import flake_amd
import setcases as sc
from test_recode_plan_cpu import build, run

V = flake_amd
BUF = 1 << 40


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return build(tmp_path_factory.mktemp("rplan_sets"), "dump", [])


@pytest.mark.parametrize("name", sc.NAMES)
def test_sources_and_witnesses_decode_to_the_pcm(name, decoder):
    c = sc.case(name)
    exp = sc.expected(c)
    ch, bps = c["ch"], c["bps"]
    for s, (x, e) in enumerate(zip(c["streams"], exp)):
        pcm, sizes = decoder.decode(x["frames"], ch, bps, len(x["pcm"]) + 1)
        assert np.array_equal(pcm, x["pcm"]) and list(sizes) == x["blocks"], (name, s)      # (its sizes count samples)
        si, hi = V.read_streaminfo(x["si_bytes"])
        assert (si.channels, si.bits_per_sample, si.sample_rate, si.samples, hi) == (ch, bps, sc.RATE, len(x["pcm"]), 0)
        assert (si.min_block_size, si.max_block_size) == (min(x["blocks"]), max(x["blocks"])) and bytes(si.md5sum) == x["md5"]
        assert V.write_streaminfo(si) == x["si_bytes"]
        got = V.index_frames(si, x["frames"])
        assert got is not None and list(got[0]) == list(x["sizes"]) and got[1] == len(x["frames"]), (name, s)
        # the witness of the recode: the same samples, cut at B
        if s not in c["named"]:
            assert e["all"] == b"" and V.read_streaminfo(e["si"])[0].samples == 0
            continue
        back, bsizes = decoder.decode(np.frombuffer(e["all"], np.uint8), ch, bps, len(x["pcm"]) + 1)
        assert np.array_equal(back, x["pcm"]) and list(bsizes) == [f[1] for f in e["frames"]], (name, s)
        assert e["all"].startswith(e["whole"]) and sum(e["block_bytes"]) == len(e["all"])
        esi, _ = V.read_streaminfo(e["si"])
        assert (esi.samples, esi.max_block_size, bytes(esi.md5sum)) == (len(x["pcm"]), c["B"], x["md5"])
        assert esi.max_frame_size >= max(f[0] for f in e["frames"])
        got = V.index_frames(esi, e["all"])
        assert list(got[0]) == [f[0] for f in e["frames"]] and got[1] == len(e["all"]), (name, s)


@pytest.mark.parametrize("name", sc.names("F1"))
def test_f1_lengths(name):
    c = sc.case(name)
    B = c["B"]
    assert [len(x["pcm"]) for x in c["streams"][:4]] == [1, B - 1, 2 * B, 2 * B + 1] and c["named"] == [0, 1, 2, 3]
    assert all(x["blocks"][:-1] == [sc.F1_SRC] * (len(x["blocks"]) - 1) for x in c["streams"])
    assert c["streams"][3]["blocks"][-1] == 1 and c["src_max"] == sc.F1_SRC
    assert sc.want_decode_batches(c) > len(c["calls"]) >= 3 and len(c["streams"]) == 5


def ids(buf, src, count):
    return buf * BUF + np.arange(src, src + count, dtype=np.int64)


def expand(pieces):
    """A piece table as the source sample (buf * 2^40 + index) at destination 0, 1, ...; it tiles its destination."""
    at, out = 0, [np.zeros(0, np.int64)]
    for buf, count, src, dst in pieces:
        assert count >= 1 and dst == at
        out.append(ids(buf, src, count))
        at += count
    return np.concatenate(out)


def restated(state, B, segs):
    """One step in numpy: every stream's carry and segments put together and cut at multiples of B."""
    blocks, owner, carry, after = [np.zeros(0, np.int64)], [], [np.zeros(0, np.int64)], []
    for s, (off, ln, _) in enumerate(state):
        mine = np.concatenate([ids(sc.CARRY, off, ln)] + [ids(sc.DEC, st, m) for t, st, m in segs if t == s])
        nb = len(mine) // B
        blocks.append(mine[:nb * B])
        owner += [s] * nb
        after.append((sum(len(x) for x in carry), len(mine) - nb * B, 0))
        carry.append(mine[nb * B:])
    return np.concatenate(blocks), owner, np.concatenate(carry), after


def walk(exe, c):
    """The planner over every step of the case, each fed the carries of the one before, against the restatement.
    Returns per step (block pieces, the blocks' streams, the state before, segments, the frames' starts)."""
    state = [(0, 0, 0)] * len(c["streams"])
    out = []
    for segs, starts in sc.steps_of(c):
        blocks, owner, carry, after = restated(state, c["B"], segs)
        got = run(exe, state, c["B"], [(s, st, m, 1) for s, st, m in segs], block_cap=len(owner))
        assert not got["refused"] and got["B"] == owner and got["S"] == after
        assert np.array_equal(expand(got["P"]), blocks) and np.array_equal(expand(got["C"]), carry)
        out.append((got["P"], owner, state, segs, starts))
        state = after
    # what is left is the tails
    assert [ln for _, ln, _ in state] == [len(x["pcm"]) % c["B"] if s in c["named"] else 0 for s, x in enumerate(c["streams"])]
    return out


@pytest.mark.parametrize("name", sc.names("F2"))
def test_f2_pieces(name, plain):
    c = sc.case(name)
    ch, B = c["ch"], c["B"]
    src = max(c["streams"][0]["blocks"])
    assert c["streams"][1]["vbs"] and c["streams"][1]["blocks"][0] == 1151 and not any(c["streams"][s]["vbs"] for s in (0, 2, 3))
    M = max(src, B)
    assert all(3 * M < len(x["pcm"]) < 5 * M and len(x["pcm"]) % B and len(x["pcm"]) % src for x in c["streams"])
    # several whole source frames in every fixed stream (the splitter cuts the other's blocks where it likes)
    assert all(sum(1 for m in x["blocks"] if m == src) >= 3 for x in c["streams"] if not x["vbs"]) and len(c["streams"][1]["blocks"]) > 3
    steps = walk(plain, c)
    longest, inside, skewed, spans = 0, 0, 0, 0
    for pieces, owner, state, segs, starts in steps:
        for buf, count, s0, dst in pieces:
            longest = max(longest, count * ch)
            if buf == sc.DEC:
                inside += s0 not in starts or s0 + count not in starts + [segs[-1][1] + segs[-1][2]]
                spans += count * ch > 1024 and count >= B
                if owner[dst // B] == 1 and (s0 * ch) % 4 != (dst * ch) % 4:
                    skewed += 1
    if (src, B) == (4096, 1152):
        assert inside > 0                  # blocks of 1152 out of frames of 4096: pieces are cut inside source frames
    else:
        assert longest > 1024, longest     # longer than one tile of K9's
    if (src, B) == (4096, 4096):
        assert spans > 0                   # a whole block as one piece: several tiles
    assert skewed > 0                      # the odd first frame: source and destination disagree modulo 16 bytes


def absent_while_carrying(c, steps):
    """The longest stretch of steps without a segment of the case's absent stream while it holds a carry."""
    best = cur = 0
    for _, _, state, segs, _ in steps:
        cur = cur + 1 if state[c["absent"]][1] > 0 and all(s != c["absent"] for s, _, _ in segs) else 0
        best = max(best, cur)
    return best


def test_f3_carries_live_long(plain):
    c = sc.case("F3-3")
    steps = walk(plain, c)
    first_block = next(i for i, st in enumerate(steps) if st[1])
    assert first_block >= 18, first_block               # 2048 / (7 * 16) = 18.3 steps for a stream that got every frame
    assert absent_while_carrying(c, steps) >= 10
    assert len(steps) == sc.want_decode_batches(c) > 60


def test_f3_seventy_streams(plain):
    c = sc.case("F3-70")
    assert absent_while_carrying(c, walk(plain, c)) >= 10
    tails = sum(1 for x in c["streams"] if len(x["pcm"]) % c["B"])
    assert len(c["streams"]) == 70 > 64 and 64 < tails < 70 and tails > c["batch"]      # some streams end on a block
    assert all(len(x["pcm"]) >= c["B"] for x in c["streams"])


def test_f4_holds_the_forms_this_encoder_never_writes():
    kinds, assignments, blocking = set(), set(), set()
    for name in sc.names("F4"):
        c = sc.case(name)
        for x in c["streams"]:
            kinds |= set(x["forms"])
            blocking.add(x["vbs"])
            for a in x["off"][:-1]:
                assignments.add((c["ch"], int(x["frames"][a + 3]) >> 4))
                assert (int(x["frames"][a + 1]) & 1) == x["vbs"]
    assert {(2, 1), (2, 8), (2, 9), (2, 10), (1, 0), (3, 2)} <= assignments and blocking == {False, True}
    # (the forms as they were handed to flacgen.frame, after the stereo and short-block replacements)
    assert {("constant", 0, 0, 0, False), ("verbatim", 0, 0, 0, False), ("lpc", 4, 0, 0, False)} <= kinds
    assert {o for k, o, _, _, _ in kinds if k == "fixed"} == {0, 1, 2, 3, 4}
    assert {m for _, _, m, _, _ in kinds} == {0, 1} and any(w for _, _, _, w, _ in kinds) and any(e for _, _, _, _, e in kinds)
    for name in sc.names("F4"):            # every set has FIXED order 0, every side-coded stream is free of CONSTANT and wasted bits
        c = sc.case(name)
        assert any(("fixed", 0, 0, 0, False) in x["forms"] for x in c["streams"]), name
        for x in c["streams"]:
            if c["ch"] == 2 and int(x["frames"][3]) >> 4 >= 8:
                assert not any(k == "constant" or w for k, _, _, w, _ in x["forms"])
    assert {sc.case(n)["B"] for n in sc.names("F4")} == {96, 4096}
    assert any(x["blocks"][0] == 16 for n in sc.names("F4") for x in sc.case(n)["streams"])


@pytest.mark.parametrize("name", sc.names("F5"))
def test_f5_every_expected_frame_is_verbatim(name):
    c = sc.case(name)
    exp = sc.expected(c)
    frames = [f for e in exp for f in e["frames"]]
    assert all(verb for _, _, verb in frames), name
    # the largest one, for the record (-s shows it)
    print(f"{name}: largest expected frame {max(size for size, _, _ in frames)} bytes, the VERBATIM threshold "
          f"{sc.verbatim_size(c['ch'], c['bps'], c['B'])}")
    # stream 0 alone fills the bound's block count: whole source frames that are whole output blocks
    x = c["streams"][0]
    assert len(x["pcm"]) % c["B"] == 0 and set(x["blocks"]) == {c["src_max"]}


def test_f5_reaches_the_splitters_eight_piece_form():
    """(Not in every format: the splitter's score wraps at 32 bits with 24-bit noise, and stereo needs noise that is
    alike in its second differences to stay VERBATIM.)"""
    eight = [n for n in sc.names("F5") if sc.case(n)["level"] == 10
             and sum(1 for _, m, _ in sc.expected(sc.case(n))[1]["frames"] if m == sc.case(n)["B"] // 8) == 8]
    assert eight, eight
