"""Seek points recorded while encoding (flake_amd_seekpoints, flake_amd_set_seekpoints, flake_amd_recode_set_seekpoints):
the points every encode path records are held to the rule restated in seekpoints_rule.py, over the block sizes the test
handed in and the byte counts the calls returned, with the first frame's samples read from the header by a parser of the
test's own.  Recording changes no frame byte and no STREAMINFO, a refused call changes no points, and the switch is
refused once a block has been committed."""
import numpy as np
import pytest
import torch as _torch

import flake_amd
from seekpoints_rule import as_tuples, header_at, rule
from test_gpu_decode_set import as_call, encode_set, round_robin

pytestmark = pytest.mark.gpu

V = flake_amd
LENS = [64 * 30 + 13, 64 * 25, 64 * 3 + 1]
VBS_LENS = [256 * 6 + 100, 256 * 2]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def pcm_of(lens, seed):
    return [np.ascontiguousarray(V.synth_pcm(1, n, 2, 16, first_frame=seed + s).reshape(-1, 2), np.int32) for s, n in enumerate(lens)]


def through_a_set(pcms, bs, level, flags, spacing, dtype=np.int32, verify=False):
    """The streams through one StreamSet: whole blocks round-robin in two calls, the tails in one ragged call.  Per
    stream: its frame bytes, its blocks as (samples, bytes), its STREAMINFO (struct and bytes), its points."""
    S = len(pcms)
    frames, blocks = [b""] * S, [[] for _ in range(S)]
    with V.StreamSet(S, level=level, flags=flags, block_size=bs) as st:
        st.set_verify(verify)
        if spacing:
            st.seekpoints(spacing)
        order = sorted((j, s) for s in range(S) for j in range(len(pcms[s]) // bs))
        calls = [order[:len(order) // 2], order[len(order) // 2:]]
        tails = [(s, len(pcms[s]) % bs) for s in range(S) if len(pcms[s]) % bs]
        for part in calls:
            out, sizes = st.encode(np.concatenate([pcms[s][j * bs:(j + 1) * bs] for j, s in part]), bs, [s for _, s in part], dtype=dtype)
            at = 0
            for (j, s), n in zip(part, sizes):
                frames[s] += out[at:at + n].tobytes()
                blocks[s].append((bs, int(n)))
                at += n
        out, sizes = st.encode_ragged(np.concatenate([pcms[s][len(pcms[s]) - t:] for s, t in tails]), [t for _, t in tails],
                                      [s for s, _ in tails], dtype=dtype)
        at = 0
        for (s, t), n in zip(tails, sizes):
            frames[s] += out[at:at + n].tobytes()
            blocks[s].append((t, int(n)))
            at += n
        return dict(frames=frames, blocks=blocks, si=[st.streaminfo(s) for s in range(S)],
                    si_bytes=[st.streaminfo_bytes(s) for s in range(S)],
                    points=[as_tuples(st.get_seekpoints(s)) for s in range(S)])


def expected(frames, blocks, spacing):
    """The rule over the blocks, each block's first frame read from the header where the block starts."""
    at, rows = 0, []
    for samples, nbytes in blocks:
        rows.append((samples, nbytes, header_at(frames, at)[0]))
        at += nbytes
    assert at == len(frames)
    return rule(rows, spacing)


_plain = {}


def plain(key, make):
    if key not in _plain:
        _plain[key] = make()
    return _plain[key]


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("flags", [0, V.SET_MD5_HOST])
@pytest.mark.parametrize("dtype", [np.int32, np.int16])
def test_stream_set_level_5(dtype, flags, verify):
    pcms = pcm_of(LENS, 300)
    off = plain(("fixed", dtype, flags, verify), lambda: through_a_set(pcms, 64, 5, flags, 0, dtype, verify))
    assert off["points"] == [[], [], []]
    for spacing in (64, 200, 10000):
        on = through_a_set(pcms, 64, 5, flags, spacing, dtype, verify)
        assert on["frames"] == off["frames"] and on["si_bytes"] == off["si_bytes"]          # recording changes no bytes
        for s in range(len(LENS)):
            want = expected(on["frames"][s], on["blocks"][s], spacing)
            assert on["points"][s] == want, (spacing, s)
            assert want[0] == (0, 0, min(64, LENS[s])) and all(p[2] == min(64, LENS[s] - p[0]) for p in want)
            sizes, used = V.index_frames(on["si"][s], on["frames"][s])
            starts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
            assert used == len(on["frames"][s])
            for sample, offset, _ in on["points"][s]:
                assert offset in starts and starts.index(offset) == sample // 64
        assert len(on["points"][0]) == {64: 31, 200: 10, 10000: 1}[spacing]


@pytest.mark.parametrize("ragged", ["1", "0"])
def test_stream_set_level_10(monkeypatch, ragged):
    monkeypatch.setenv("FLAKE_AMD_SET_RAGGED", ragged)
    pcms = pcm_of(VBS_LENS, 400)
    off = plain(("vbs", ragged), lambda: through_a_set(pcms, 256, 10, V.SET_VBS, 0))
    for spacing in (300, 256):
        on = through_a_set(pcms, 256, 10, V.SET_VBS, spacing)
        assert on["frames"] == off["frames"] and on["si_bytes"] == off["si_bytes"]
        for s in range(len(VBS_LENS)):
            assert on["points"][s] == expected(on["frames"][s], on["blocks"][s], spacing), (spacing, s)
            for sample, offset, frame_samples in on["points"][s]:
                n, number, vbs = header_at(on["frames"][s], offset)
                assert (n, number, vbs) == (frame_samples, sample, 1)
        assert [p[0] for p in on["points"][0]] == ([0, 256, 512, 768, 1024, 1280, 1536] if spacing == 256
                                                   else [0, 256, 512, 768, 1024, 1280])
    # the blocks were split: a point names the first of several frames
    sizes, _ = V.index_frames(off["si"][0], off["frames"][0])
    assert len(sizes) > len(off["blocks"][0])


def ragged_call(st, buf, block_sizes, streams, room):
    """flake_amd_set_encode_ragged with an output buffer of `room` bytes: (return value, frame sizes)."""
    bsz, sob = np.asarray(block_sizes, np.int32), np.asarray(streams, np.int32)
    out, sizes = np.zeros(1 << 16, np.uint8), np.zeros(len(bsz), np.int32)
    r = st.lib.flake_amd_set_encode_ragged(st._g, buf.ctypes.data, 4, len(bsz), bsz.ctypes.data, sob.ctypes.data,
                                           out.ctypes.data, room, sizes.ctypes.data)
    return r, sizes.tolist()


def test_a_refused_call_changes_no_points(monkeypatch):
    """A stream index outside the set; and the rollback of a ragged call under FLAKE_AMD_SET_RAGGED=0 whose output buffer
    holds the full blocks and the first length group of the short ones but not the second: the groups that were
    committed are taken back, their points with them."""
    monkeypatch.setenv("FLAKE_AMD_SET_RAGGED", "0")
    pcms = pcm_of(LENS, 300)
    first = np.concatenate([p[:64] for p in pcms])
    second = np.ascontiguousarray(np.concatenate([pcms[0][64:128], pcms[1][64:77], pcms[2][64:65]]))
    sets = []
    for _ in range(2):
        st = V.StreamSet(3, level=5, flags=V.SET_MD5_HOST, block_size=64)
        st.seekpoints(64)
        _, head = st.encode(first, 64, [0, 1, 2])
        sets.append(st)
    twin, st = sets
    try:
        r, sizes = ragged_call(twin, second, [64, 13, 1], [0, 1, 2], 1 << 16)          # what the call writes with room
        assert r == sum(sizes) and min(sizes) > 4
        before = [as_tuples(st.get_seekpoints(s)) for s in range(3)]
        info = [st.streaminfo_bytes(s) for s in range(3)]
        assert before == [[(0, 0, 64)]] * 3
        with pytest.raises(V.FlakeHipError):
            st.encode(first[:64], 64, [3])
        assert [as_tuples(st.get_seekpoints(s)) for s in range(3)] == before
        assert st.lib.flake_amd_set_get_seekpoints(st._g, 3, None, 0) == -1
        r, _ = ragged_call(st, second, [64, 13, 1], [0, 1, 2], sizes[0] + sizes[1] + 4)
        assert r == -1 and "too small" in st.last_error()
        assert [as_tuples(st.get_seekpoints(s)) for s in range(3)] == before
        assert [st.streaminfo_bytes(s) for s in range(3)] == info
        r, again = ragged_call(st, second, [64, 13, 1], [0, 1, 2], 1 << 16)            # nothing was lost: the same call goes through
        assert r == sum(sizes) and again == sizes
        for s, n in enumerate((64, 13, 1)):
            want = [(0, 0, 64), (64, int(head[s]), n)]
            assert as_tuples(st.get_seekpoints(s)) == as_tuples(twin.get_seekpoints(s)) == want
    finally:
        twin.close(), st.close()


def test_the_switch_is_refused_after_the_first_block():
    lib = V.load_host_library()
    pcm = pcm_of([128], 7)[0]
    with V.StreamSet(2, level=5, block_size=64) as st:
        st.seekpoints(64), st.seekpoints(0), st.seekpoints(1000)            # before the first block: as often as one likes
        st.encode(pcm[:64], 64, [1])
        assert lib.flake_amd_set_seekpoints(st._g, 64) == -1
        with pytest.raises(RuntimeError):
            st.seekpoints(0)
        st.encode(pcm[64:], 64, [1])
        assert as_tuples(st.get_seekpoints(1)) == [(0, 0, 64)] and len(st.get_seekpoints(0)) == 0      # the last spacing, 1000, held
    with V.HostEncoder(5, block_size=64) as enc:
        enc.seekpoints(64)
        enc.encode_frames(pcm[:64], 64, 0)
        assert lib.flake_amd_seekpoints(enc.ctx, 64) == -1
    assert lib.flake_amd_set_seekpoints(None, 64) == -1 and lib.flake_amd_seekpoints(None, 64) == -1
    assert lib.flake_amd_recode_set_seekpoints(None, 64) == -1
    assert lib.flake_amd_set_get_seekpoints(None, 0, None, 0) == -1 and lib.flake_amd_get_seekpoints(None, None, 0) == -1


@pytest.mark.parametrize("level, bs, calls, tail, spacings", [(5, 64, (10, 20), 13, (64, 200, 10000)),
                                                              (10, 256, (3, 3), 100, (300, 256))])
def test_host_encoder(level, bs, calls, tail, spacings):
    n0, n1 = calls
    pcm = pcm_of([(n0 + n1) * bs + tail], 500)[0]

    def run(spacing):
        with V.HostEncoder(level, block_size=bs) as enc:
            if spacing:
                enc.seekpoints(spacing)
            a, sa = enc.encode_frames(pcm[:n0 * bs], bs, 0)
            b, sb = enc.encode_frames(pcm[n0 * bs:], bs, tail)
            return a.tobytes() + b.tobytes(), [int(n) for n in list(sa) + list(sb)], as_tuples(enc.get_seekpoints()), \
                V.write_streaminfo(enc.streaminfo())

    frames, sizes, none, info = run(0)
    assert none == []
    blocks = list(zip([bs] * (n0 + n1) + [tail], sizes))
    for spacing in spacings:
        got_frames, got_sizes, points, got_info = run(spacing)
        assert (got_frames, got_sizes, got_info) == (frames, sizes, info)
        assert points == expected(frames, blocks, spacing), spacing
        for sample, offset, frame_samples in points:
            n, number, vbs = header_at(frames, offset)
            assert n == frame_samples and number == (sample if level == 10 else sample // bs) and vbs == (level == 10)
    assert len(expected(frames, blocks, spacings[0])) > 5


def test_host_encoder_look_ahead(monkeypatch):
    """flake_amd_encode_frame under FLAKE_AMD_LOOKAHEAD=4: blocks are queued, and recorded when the queue is flushed."""
    monkeypatch.setenv("FLAKE_AMD_LOOKAHEAD", "4")
    total = 64 * 9 + 13
    pcm = pcm_of([total], 600)[0]
    frames = b""
    with V.HostEncoder(5, block_size=64, samples=total) as enc:
        enc.seekpoints(200)
        for b in range(10):
            got = enc.encode_frame(pcm[b * 64:(b + 1) * 64])
            frames += got
            if b == 2:
                assert got == b"" and len(enc.get_seekpoints()) == 0       # three blocks queued: nothing is committed yet
            if b == 3:
                assert got != b"" and [p[0] for p in enc.get_seekpoints()] == [0, 192]       # the flush of four blocks
        points = as_tuples(enc.get_seekpoints())
        si = enc.streaminfo()
    sizes, used = V.index_frames(si, frames)
    assert used == len(frames) and len(sizes) == 10
    assert points == rule(list(zip([64] * 9 + [13], map(int, sizes), [64] * 9 + [13])), 200)
    assert [p[0] for p in points] == [0, 192, 384]            # (the tail, 576 .. 589, holds no target)


@pytest.mark.parametrize("bs, level, flags", [(96, 5, 0), (256, 10, V.SET_VBS)])
def test_recode_set(bs, level, flags):
    src = plain("sources", lambda: encode_set(LENS, 64, 5, 0, 300))
    pcms = [x["pcm"] for x in src]
    want = through_a_set(pcms, bs, level, flags, 150)
    like = V.HostStreaminfo(min_block_size=64, max_block_size=64, sample_rate=44100, channels=2, bits_per_sample=16)
    runs = round_robin(src, 3)
    got = [b""] * len(src)
    with V.RecodeSet(like, len(src), level=level, flags=flags, block_size=bs) as rs:
        rs.seekpoints(150)
        for s, data in rs.recode_runs(as_call(src, runs[:len(runs) // 2])) + rs.recode_runs(as_call(src, runs[len(runs) // 2:])):
            got[s] += data
        for s, data in rs.finish():
            got[s] += data
        assert got == want["frames"]
        for s in range(len(src)):
            assert as_tuples(rs.get_seekpoints(s)) == want["points"][s], s
            assert rs.streaminfo_bytes(s)[:18] == want["si_bytes"][s][:18]         # (the digest is the decode side's)
        assert rs.lib.flake_amd_recode_set_get_seekpoints(rs._g, len(src), None, 0) == -1
    assert [p[0] for p in want["points"][1]] == ([0, 96, 288, 384, 576, 672, 864, 960, 1152, 1344, 1440] if bs == 96
                                                 else [0, 256, 512, 768, 1024, 1280])
    # a stream that fails has no points; the others have all of theirs
    bad = [x["frames"] for x in src]
    bad[1] = bad[1].copy()
    bad[1][src[1]["off"][4] + src[1]["sizes"][4] // 2] ^= 0x08
    with V.RecodeSet(like, len(src), level=level, flags=flags, block_size=bs) as rs:
        rs.seekpoints(150)
        rs.recode_runs(as_call(src, runs, bad))
        rs.finish()
        assert rs.failed(1) is not None and rs.get_seekpoints(1) is None
        assert rs.lib.flake_amd_recode_set_get_seekpoints(rs._g, 1, None, 0) == -1
        assert [as_tuples(rs.get_seekpoints(s)) for s in (0, 2)] == [want["points"][0], want["points"][2]]
