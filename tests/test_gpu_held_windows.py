"""Held streams (DecodeSet.hold / hold_add / held_windows / held_windows_rows) against the path they replace: value for
value what decode_windows and decode_windows_rows of the same set return when each window is asked of the whole run of
its stream, with the frames the set's own indexer finds.  Four kinds of stream -- stereo 16-bit fixed blocks of 1152, a
level-10 variable-block stream, mono 8-bit, 8 channels of 24 bits in blocks of 256 -- with FLAKE_AMD_BATCH=3 so that
device batches cut windows; windows inside a frame, across 2 and 5 frames, at sample 0, ending at, crossing and behind
the stream's end, of count 0, two on one stream, and on a stream held twice.  Damaged streams, refusals that leave the
output untouched, and the link condition: a held call uploads its tables and 12 bytes a frame, never the stream.
Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flacgen
import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
BATCH = 3
KINDS = {  # name: (level, channels, bits, block, whole blocks, tail)
    "stereo16_fixed1152": (5, 2, 16, 1152, 14, 500),
    "stereo16_level10": (10, 2, 16, 4096, 10, 1000),
    "mono8": (5, 1, 8, 576, 14, 77),
    "eight24_256": (5, 8, 24, 256, 14, 100),
}
NP_DT = {_torch.int32: np.int32, _torch.int16: np.int16, _torch.float32: np.float32}


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(autouse=True)
def small_batches(monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))


class Made:
    """One encoded stream: its bytes from the first frame header on, its STREAMINFO, its length in samples."""

    def __init__(self, kind, seed=0):
        level, ch, bps, n, nb, tail = KINDS[kind]
        pcm = V.synth_pcm(nb + 1, n, ch, bps, first_frame=seed).reshape(-1, ch)[:nb * n + tail]
        with V.HostEncoder(level, ch, bps, block_size=n) as enc:
            data, _ = enc.encode_frames(pcm, n, tail)
            self.si = enc.streaminfo()
        self.bytes = np.ascontiguousarray(data)
        self.total = nb * n + tail
        self.ch, self.bps, self.n = ch, bps, n
        self.fixed = int(self.si.max_block_size) if self.si.min_block_size == self.si.max_block_size else 0


_MADE = {}


def made(kind, seed=0):
    if (kind, seed) not in _MADE:
        _MADE[kind, seed] = Made(kind, seed)
    return _MADE[kind, seed]


def windows_for(m, a, b):
    """[(held id, first sample, count)] on held streams a and b (b holds the same bytes as a)."""
    n, t = m.n, m.total
    return [(a, 3 * n + 10, 50),              # inside one frame
            (a, 4 * n - 20, 60),              # across 2 frames
            (a, 5 * n + 7, 4 * n),            # across 5 frames (fixed blocks): more than a device batch
            (a, 0, 100),                      # at sample 0
            (a, t - 70, 70),                  # ending at the stream's end
            (a, t - 30, 100),                 # crossing it
            (a, t + 5, 10),                   # behind it
            (a, 100, 0),                      # count 0
            (b, 3 * n + 10, 50),              # the same stream, held twice
            (b, 2 * n, n + 1)]


def as_runs(wins, streams):
    """The held windows as decode_windows takes them: each asked of its stream's whole run.  streams: id -> (bytes,
    frame sizes, fixed block size)."""
    return [(*streams[i], first, count) for i, first, count in wins]


def open_set(m, streams_bytes, fixed=None):
    """A set that holds streams_bytes, and id -> (bytes, the frames the set's indexer finds, fixed block size)."""
    g = V.DecodeSet(m.si, 1, V.SET_MD5_OFF)
    g.hold(sum(len(b) for b in streams_bytes) + 64)
    fx = [m.fixed] * len(streams_bytes) if fixed is None else fixed
    ids = g.hold_add(streams_bytes, fixed_block_sizes=fx)
    found = g.index(streams_bytes)
    table = {}
    for i, b, f, x in zip(ids, streams_bytes, found, fx):
        table[i] = (b[:0], np.zeros(0, np.int32), x) if f is None else (b[:f[1]], f[0], x)      # (a run is its frames' bytes)
    return g, ids, table


def same_windows(got, want):
    (res, status, decoded, begins), (wres, wstatus, wdecoded, wbegins) = got, want
    assert list(status) == list(wstatus) and decoded == wdecoded and begins == wbegins
    for w, (r, x) in enumerate(zip(res, wres)):
        assert (r is None) == (x is None), w
        if r is not None:
            assert r.dtype == x.dtype and np.array_equal(r, x), w


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_held_windows_are_the_windows_of_the_whole_run(kind):
    m = made(kind)
    g, ids, table = open_set(m, [m.bytes, m.bytes])
    with g:
        assert ids == [0, 1]
        frames, samples, nbytes = g.held_info(0)
        assert frames == len(table[0][1]) > 6 and samples == m.total and nbytes == len(table[0][0]) == len(m.bytes)
        assert g.held_info(1) == (frames, samples, nbytes)
        stats = g.held_stats()
        assert stats[0] == 2 * len(m.bytes) and stats[1] == 2 * frames and stats[2] >= stats[0] and stats[3] == 0
        wins = windows_for(m, 0, 1)
        runs = as_runs(wins, table)
        for sample_bytes in ((4, 2) if m.bps <= 16 else (4,)):
            want = g.decode_windows(runs, sample_bytes=sample_bytes)
            before = g.device_batches()
            got = g.held_windows(wins, sample_bytes=sample_bytes)
            same_windows(got, want)
            assert g.device_batches() - before == -(-got[2] // BATCH) > 2         # batches cut the five-frame window
            # the samples are the stream's
            assert [len(r) for r in got[0]] == [50, 60, 4 * m.n, 100, 70, 30, 0, 0, 50, m.n + 1]
        assert g.held_stats()[3] > 0 and g.held_stats()[:3] == stats[:3]
        row_len = 4 * m.n + 3
        for dtype in (_torch.int32, _torch.int16, _torch.float32):
            if dtype == _torch.int16 and m.bps > 16:
                continue
            wrows, wlen, wstatus, wdecoded = g.decode_windows_rows(runs, row_len, dtype)
            out = _torch.full((len(wins) + 2, m.ch, row_len), 77, dtype=dtype, device="cuda")
            rows, glen, gstatus, gdecoded = g.held_windows_rows(wins, row_len, out=out)
            assert rows.dtype == dtype and list(gstatus) == list(wstatus) and gdecoded == wdecoded
            assert glen.tolist() == wlen.tolist()
            assert np.array_equal(rows.cpu().numpy(), wrows.cpu().numpy())
            assert (out[len(wins):].cpu().numpy() == 77).all()                     # rows behind the call's are not touched
            assert rows.cpu().numpy().any()


def test_no_windows_and_an_empty_set_of_ids():
    m = made("mono8")
    g, ids, table = open_set(m, [m.bytes])
    with g:
        res, status, decoded, begins = g.held_windows([])
        assert res == [] and decoded == 0


def damaged(m, sizes):
    """Copies of a fixed-block stereo stream: a residual bit flipped in frame 9; a header bit flipped at frame 7, which
    the bisection of a window in frame 3 of the whole stream probes (15 frames: 7, 3, ...); a header bit flipped at frame
    12, which it does not; a stream that does not begin with a header; and frame 9 with the reserved bit of its first
    subframe header set and its CRC-16 made good again, which only the decoder can refuse."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    crc = m.bytes.copy()
    crc[off[10] - 4] ^= 0x02
    probed = m.bytes.copy()
    probed[off[7] + 2] ^= 0x10                 # the block-size code: the CRC-8 fails
    unprobed = m.bytes.copy()
    unprobed[off[12] + 2] ^= 0x10
    refused = m.bytes.copy()
    refused[0] ^= 0x01
    syntax = m.bytes.copy()
    syntax[off[9] + 6] |= 0x80                 # (the header of a stereo frame of 1152 at 44.1 kHz takes six bytes)
    syntax[off[10] - 2:off[10]] = np.frombuffer(flacgen.crc16(bytes(syntax[off[9]:off[10] - 2])).to_bytes(2, "big"), np.uint8)
    return crc, probed, unprobed, refused, syntax


def test_damage_fails_what_it_fails_on_the_parent_path():
    """What damage does to a held stream.  The set's table comes from K8, which takes a frame only with a header the
    predicate accepts and a CRC-16 that holds: a flipped residual bit or header bit therefore ENDS the held stream in
    front of the frame (as it ends the run the indexer finds, which is what the parent path is asked of), and a window
    there delivers what is left, with status 0 -- never CRC16 or HEADER, which need a table that disagrees with the bytes
    (tests/test_held_plan_cpu.py holds the planner to HEADER exactly where the byte planner says it; the ABI test below
    holds the device entry to CRC16 on a store damaged behind its table).  A frame that K8 takes and K7 refuses fails its
    window alone, its row zero."""
    m = made("stereo16_fixed1152")
    with V.DecodeSet(m.si, 1, V.SET_MD5_OFF) as g0:
        sizes = g0.index([m.bytes])[0][0]
    assert len(sizes) == 15
    copies = damaged(m, sizes)
    n = m.n
    g, ids, table = open_set(m, [m.bytes, *copies])
    with g:
        good, crc, probed, unprobed, refused, syntax = ids
        assert [g.held_info(i)[0] for i in ids] == [15, 9, 6, 11, 0, 15]
        assert [len(table[i][1]) for i in ids] == [15, 9, 6, 11, 0, 15]             # the indexer's runs are the same
        assert g.held_info(refused) == (0, 0, 0)
        wins = [(good, 3 * n + 10, 50), (syntax, 8 * n + 5, 2 * n), (good, 8 * n + 5, 2 * n), (syntax, 3 * n + 10, 50),
                (crc, 3 * n + 10, 50), (crc, 8 * n + 5, 2 * n), (crc, 10 * n, 50),
                (probed, 3 * n + 10, 50), (probed, 7 * n + 10, 50), (probed, 5 * n + 10, 3 * n),
                (unprobed, 3 * n + 10, 50), (unprobed, 10 * n, 3 * n), (refused, 0, 100), (refused, 3 * n, 10),
                (good, 0, 20)]
        runs = as_runs(wins, table)
        want = g.decode_windows(runs)
        got = g.held_windows(wins)
        same_windows(got, want)
        res, status, decoded, begins = got
        print("statuses:", list(status))
        assert status[1] != 0 and res[1] is None                                  # the window fails alone
        assert list(status[:1]) + list(status[2:]) == [0] * (len(wins) - 1)
        assert [len(r) for r in res[2:]] == [2 * n, 50, 50, n - 5, 0, 50, 0, n - 10, 50, n, 0, 0, 20]
        row_len = 3 * n
        wrows, wlen, wstatus, _ = g.decode_windows_rows(runs, row_len, _torch.int32)
        rows, glen, gstatus, _ = g.held_windows_rows(wins, row_len, _torch.int32)
        assert list(gstatus) == list(wstatus) == list(status) and glen.tolist() == wlen.tolist()
        got_rows = rows.cpu().numpy()
        assert np.array_equal(got_rows, wrows.cpu().numpy())
        assert glen[1] == -1 and not got_rows[1].any() and got_rows[2].any()        # the failed window's row is zero


def test_refusals_leave_everything_as_it_was():
    m = made("stereo16_fixed1152")
    g, ids, table = open_set(m, [m.bytes])
    with g:
        stats = g.held_stats()
        out = np.full((64, 2), -77, np.int32)
        for wins in ([(1, 0, 10)], [(-1, 0, 10)], [(0, 0, 10), (7, 0, 10)], [(0, 0, -1)], [(0, 0, 65)]):
            with pytest.raises(V.FlakeHipError):
                g.held_windows(wins, pcm_cap=64, out=out)
            assert (out == -77).all(), (wins, g.last_error())
        rows = _torch.full((2, 2, 32), 77, dtype=_torch.int32, device="cuda")
        for wins in ([(0, 0, 33)], [(5, 0, 10)], [(0, 0, 10), (0, 5, -2)]):
            with pytest.raises(V.FlakeHipError):
                g.held_windows_rows(wins, 32, out=rows)
            assert (rows.cpu().numpy() == 77).all(), (wins, g.last_error())
        with pytest.raises(V.FlakeHipError):
            g.hold(1 << 20)                                                       # a second store
        with pytest.raises(V.FlakeHipError):
            g.hold_add([m.bytes])                                                 # 64 bytes are left
        assert g.held_stats() == stats
        with pytest.raises(IndexError):
            g.held_info(1)
        res, status, decoded, _ = g.held_windows([(0, 5, 10)])
        assert decoded == 1 and len(res[0]) == 10 and list(status) == [0]
    with V.DecodeSet(m.si, 1, V.SET_MD5_OFF) as bare:
        with pytest.raises(V.FlakeHipError):
            bare.hold_add([m.bytes])                                              # no store
        with pytest.raises(V.FlakeHipError):
            bare.held_windows([(0, 0, 10)])
        with pytest.raises(V.FlakeHipError):
            bare.hold(0)


def noise_streams(nstreams, nframes, n=4096, seed=5):
    r = np.random.RandomState(seed)
    out = []
    for _ in range(nstreams):
        pcm = r.randint(-32768, 32768, size=(nframes * n, 2)).astype(np.int32)
        with V.HostEncoder(5, 2, 16, block_size=n) as enc:                     # (a stream of its own: numbered from 0)
            out.append(np.ascontiguousarray(enc.encode_frames(pcm, n, 0)[0]))
            si = enc.streaminfo()
    return out, si


def test_the_link_carries_tables_not_streams(monkeypatch):
    """64 windows of 2 frames of noise, stereo 16-bit blocks of 4096 (about 16 KB a frame): the held call uploads at most
    128 bytes per frame and 8192 per device batch, below 1/20 of the frame bytes K7 is handed."""
    monkeypatch.delenv("FLAKE_AMD_BATCH")
    n = 4096
    streams, si = noise_streams(8, 9)
    with V.DecodeSet(si, 1, V.SET_MD5_OFF) as g:
        g.hold(sum(len(s) for s in streams))
        ids = g.hold_add(streams, fixed_block_sizes=[n] * 8)
        found = g.index(streams)
        sizes = np.concatenate([f[0] for f in found])
        assert len(sizes) == 72 and sizes.min() > 15000 and sizes.max() < 18000    # about 16 KB each
        wins = [(ids[s], k * n + n // 2, n) for s in range(8) for k in range(8)]
        want = g.decode_windows([(streams[s], found[s][0], n, first, count) for s, first, count in wins])
        before, batches = g.held_stats()[3], g.device_batches()
        got = g.held_windows(wins)
        grown, batches = g.held_stats()[3] - before, g.device_batches() - batches
        same_windows(got, want)
        decoded = got[2]
        assert [len(r) for r in got[0]] == [n] * 64
        assert decoded == 128 and batches == 1
        handed = sum(int(found[s][0][k]) + int(found[s][0][k + 1]) for s in range(8) for k in range(8))
        print(f"held call: {grown} bytes uploaded for {decoded} frames ({handed} frame bytes) in {batches} batch")
        assert 0 < grown <= 128 * decoded + 8192 * batches
        assert grown * 20 < handed
        before = g.held_stats()[3]
        g.held_windows_rows(wins, n)
        assert 0 < g.held_stats()[3] - before <= 128 * decoded + 8192 * batches


def test_the_abi_entries_gather_then_decode():
    """fhip_decode_frames_windows_held and _rows_held on a store of two copies of a stream: the launch list is the two
    gather kernels followed by the host form's, and every output is the host form's."""
    m = made("stereo16_fixed1152")
    with V.DecodeSet(m.si, 1, V.SET_MD5_OFF) as g0:
        sizes = g0.index([m.bytes])[0][0]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, pad = m.n, 13
    store = _torch.from_numpy(np.concatenate([np.zeros(pad, np.uint8), m.bytes, m.bytes])).cuda()
    nbytes = pad + 2 * len(m.bytes)
    # two segments: frames 2 .. 5 of the first copy (skip 100, take 3000), frames 9 .. 10 of the second
    pick = [(0, 2, 6), (1, 9, 11)]
    f_src = np.concatenate([pad + c * len(m.bytes) + off[a:b] for c, a, b in pick])
    f_len = np.concatenate([sizes[a:b] for c, a, b in pick]).astype(np.int32)
    host_stream = np.concatenate([m.bytes[off[a]:off[b]] for c, a, b in pick])
    seg_first, seg_number, skip, take = [0, 4, 6], [2, 9], [100, 0], [3000, -1]
    cap = 6 * n
    p = V.level_params(5, block_size=n)
    with V.Encoder(p, max_frames=8) as enc:
        want = enc.decode_frames_windows(host_stream, f_len, cap, seg_first, skip, take, seg_number)
        host_list = enc.last_launches()
        got = enc.decode_frames_windows_held(store, nbytes, f_src, f_len, cap, seg_first, skip, take, seg_number)
        assert enc.last_launches() == ["k_gather_offsets", "k_gather_frames"] + host_list
        assert got[0] == want[0] == V.OK and got[2] == want[2] == 3000 + 2 * n
        assert np.array_equal(got[1], want[1])
        for a, b in zip(got[3:8], want[3:8]):
            assert np.array_equal(a, b)
        # a damaged frame fails its segment alone, as in the host form
        hurt = store.clone()
        hurt[int(f_src[5]) + int(f_len[5]) - 4] ^= 2
        bad_host = host_stream.copy()
        bad_host[int(f_len[:6].sum()) - 4] ^= 2
        want = enc.decode_frames_windows(bad_host, f_len, cap, seg_first, skip, take, seg_number)
        got = enc.decode_frames_windows_held(hurt, nbytes, f_src, f_len, cap, seg_first, skip, take, seg_number)
        assert got[0] == want[0] == V.E_VERIFY and got[8] == want[8]
        for a, b in zip(got[3:8], want[3:8]):
            assert np.array_equal(a, b)
        # rows
        rows_w = _torch.zeros((2, 2, 3000), dtype=_torch.float32, device="cuda")
        rows_g = _torch.zeros((2, 2, 3000), dtype=_torch.float32, device="cuda")
        want = enc.decode_frames_windows_rows(host_stream, f_len, cap, seg_first, skip, take, [0, 1], [0, 0], rows_w, 2, 3000,
                                              V.ROWS_F32, seg_number)
        host_list = enc.last_launches()
        got = enc.decode_frames_windows_rows_held(store, nbytes, f_src, f_len, cap, seg_first, skip, take, [0, 1], [0, 0],
                                                  rows_g, 2, 3000, V.ROWS_F32, seg_number)
        assert enc.last_launches() == ["k_gather_offsets", "k_gather_frames"] + host_list and host_list[-1] == "k_window_rows"
        assert got[0] == want[0] == V.OK and np.array_equal(rows_g.cpu().numpy(), rows_w.cpu().numpy()) and rows_g.any()
        # refusals: nothing queued, an empty launch list
        out = np.full((cap, 2), -77, np.int32)
        args = (cap, seg_first, skip, take, seg_number)
        calls = [dict(null_table=t) for t in ("src", "frame_src", "frame_len", "segs", "win")]
        for kw in calls:
            r = enc.decode_frames_windows_held(store, nbytes, f_src, f_len, *args, out=out, **kw)
            assert r[0] == V.E_INVALID and enc.last_launches() == [], kw
        for src_bytes, fs, fl in ((-1, f_src, f_len), (nbytes, f_src + len(m.bytes), f_len), (nbytes, -f_src - 1, f_len),
                                  (nbytes, f_src, -f_len), (int(f_src[0]) + 10, f_src, f_len)):
            r = enc.decode_frames_windows_held(store, src_bytes, fs, fl, *args, out=out)
            assert r[0] == V.E_INVALID and enc.last_launches() == [], (src_bytes,)
        many = 9
        r = enc.decode_frames_windows_held(store, nbytes, np.zeros(many, np.int64), np.ones(many, np.int32), cap, [0, many],
                                           [0], [-1], out=out)
        assert r[0] == V.E_INVALID and enc.last_launches() == []                  # more frames than max_frames
        assert (out == -77).all()
        enc.set_pcm_format(V.PCM_S16)
        r = enc.decode_frames_windows_rows_held(store, nbytes, f_src, f_len, cap, seg_first, skip, take, [0, 1], [0, 0],
                                                rows_g, 2, 3000, V.ROWS_F32, seg_number)
        assert r[0] == V.E_UNSUPPORTED and enc.last_launches() == []
