"""K9 (fhip_gather_spans_dev, flake_amd.Encoder.gather_spans_dev) against a numpy gather: every value where the table puts
it, nothing outside the table's destination touched, and the tables the host must refuse refused with nothing queued.
Every comparison is exact."""
import numpy as np
import pytest
import torch as _torch

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
TILE_VALS = 1024                  # interleaved values per workgroup (k9_gather.hip: 4 KiB)
BLOCK = 4096
GUARD = 64                        # sentinel values on either side of the destination
SENTINEL = -0x5A5A5A5B


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def handle(ch):
    return V.Encoder(V.level_params(5, channels=ch, bits_per_sample=16), max_frames=4)


class Bench:
    """Two sources of random samples on the device and a guarded destination."""

    def __init__(self, ch, cap0, cap1, dst_cap, seed=1):
        r = np.random.RandomState(seed)
        self.ch = ch
        self.src = [r.randint(-2 ** 31, 2 ** 31 - 1, size=(c, ch), dtype=np.int64).astype(np.int32) for c in (cap0, cap1)]
        self.dev = [_torch.from_numpy(s.copy()).cuda() if len(s) else None for s in self.src]
        self.dst_cap = dst_cap
        self.dst = _torch.full((2 * GUARD + dst_cap * ch,), SENTINEL, dtype=_torch.int32, device="cuda")
        _torch.cuda.synchronize()

    def run(self, enc, rows):
        rc = enc.gather_spans_dev(self.dst.data_ptr() + 4 * GUARD, self.dst_cap, self.dev[0], len(self.src[0]),
                                  self.dev[1], len(self.src[1]), V.gather_pieces(rows))
        launches = enc.last_launches()
        enc.sync()
        return rc, launches

    def want(self, rows):
        out = np.full(2 * GUARD + self.dst_cap * self.ch, SENTINEL, dtype=np.int32)
        body = out[GUARD:GUARD + self.dst_cap * self.ch].reshape(-1, self.ch)
        for buf, src, dst, count in rows:
            body[dst:dst + count] = self.src[buf][src:src + count]
        return out

    def got(self):
        return self.dst.cpu().numpy()

    def untouched(self):
        return bool((self.got() == SENTINEL).all())


def table(ch, cap0, cap1):
    """Pieces of every length class, each at every source residue and, through fillers of 1 .. 3 samples, every
    destination residue modulo 4 samples; both sources; one piece that ends exactly at its source's capacity."""
    tile = TILE_VALS // ch
    rows, at, k = [], 0, 0
    for n in (1, 2, 3, tile - 1, tile + 1, BLOCK):
        for sr in range(4):
            for fill in range(4):
                if fill:
                    rows.append((k & 1, 8 * k + 1, at, fill))
                    at += fill
                buf = (k >> 1) & 1
                cap = cap1 if buf else cap0
                src = (37 * k * 4) % (cap - n - 8) // 4 * 4 + sr
                rows.append((buf, src, at, n))
                at += n
                k += 1
    rows.append((0, cap0 - 77, at, 77))
    at += 77
    rows.append((1, cap1 - 1, at, 1))
    return rows, at + 1


@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_every_length_and_residue_against_numpy(ch):
    cap0, cap1 = 3 * BLOCK + 5, 2 * BLOCK + 3
    rows, total = table(ch, cap0, cap1)
    assert {(s % 4, d % 4) for _, s, d, n in rows if n >= 4} == {(a, b) for a in range(4) for b in range(4)}
    assert {b for b, *_ in rows} == {0, 1}
    assert any(s + n == cap0 for b, s, _, n in rows if b == 0) and any(s + n == cap1 for b, s, _, n in rows if b == 1)
    bench = Bench(ch, cap0, cap1, total)                   # the destination's capacity is exactly the table's total
    with handle(ch) as enc:
        rc, launches = bench.run(enc, rows)
        assert rc == V.OK and launches == ["k_gather_spans"]
        assert np.array_equal(bench.got(), bench.want(rows))
        enc.set_profiling(True)
        assert bench.run(enc, rows)[0] == V.OK
        times = enc.kernel_times()
        assert times["k_gather_spans"][1] == 1 and times["k_gather_spans"][0] > 0


@pytest.mark.parametrize("ch", [1, 3])
def test_many_one_sample_pieces_per_tile(ch):
    """More than 1024 one-sample pieces: with one channel a tile holds 1024 of them."""
    n = 2500
    r = np.random.RandomState(5)
    src = r.randint(0, 4000, n)
    rows = [(int(k & 1), int(src[k]), k, 1) for k in range(n)]
    bench = Bench(ch, 4000, 4000, n + 9)                   # ... and a destination larger than the table
    with handle(ch) as enc:
        rc, launches = bench.run(enc, rows)
        assert rc == V.OK and launches == ["k_gather_spans"]
        assert np.array_equal(bench.got(), bench.want(rows))


@pytest.mark.parametrize("ch", [2, 3])
def test_one_piece_spanning_many_tiles(ch):
    n = 5 * TILE_VALS + 3
    for rows in ([(1, 2, 0, n)], [(0, 1, 0, 3), (1, 5, 3, n), (0, 0, 3 + n, 2)]):
        total = sum(c for *_, c in rows)
        bench = Bench(ch, 64, n + 8, total)
        with handle(ch) as enc:
            assert bench.run(enc, rows) == (V.OK, ["k_gather_spans"])
            assert np.array_equal(bench.got(), bench.want(rows))


def test_an_empty_table_queues_nothing():
    bench = Bench(2, 16, 16, 16)
    with handle(2) as enc:
        assert bench.run(enc, []) == (V.OK, [])
        assert bench.untouched()
        # a source of capacity 0 may be null as long as no piece names it
        rc = enc.gather_spans_dev(bench.dst.data_ptr() + 4 * GUARD, 16, bench.dev[0], 16, None, 0, V.gather_pieces([(0, 3, 0, 5)]))
        enc.sync()
        assert rc == V.OK
        assert np.array_equal(bench.got()[GUARD:GUARD + 10].reshape(-1, 2), bench.src[0][3:8])


REFUSED = {
    "a gap": [(0, 0, 0, 4), (0, 4, 5, 4)],
    "an overlap": [(0, 0, 0, 4), (0, 4, 3, 4)],
    "unsorted": [(0, 0, 4, 4), (0, 4, 0, 4)],
    "not from 0": [(0, 0, 1, 4)],
    "a source overrun": [(0, 0, 0, 4), (1, 30, 4, 3)],
    "a negative source": [(0, -1, 0, 4)],
    "a destination overrun": [(0, 0, 0, 30), (1, 0, 30, 11)],
    "a count of 0": [(0, 0, 0, 4), (0, 4, 4, 0), (0, 8, 4, 4)],
    "a source buffer that is not 0 or 1": [(2, 0, 0, 4)],
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refused_tables_queue_nothing(what):
    bench = Bench(2, 40, 32, 40)
    with handle(2) as enc:
        assert bench.run(enc, [(0, 0, 0, 8)])[0] == V.OK    # (a launch list to be emptied)
        bench.dst.fill_(SENTINEL)
        _torch.cuda.synchronize()
        rc, launches = bench.run(enc, REFUSED[what])
        assert rc == V.E_INVALID and launches == [], what
        assert bench.untouched(), what


def test_int16_pcm_is_refused():
    bench = Bench(2, 40, 32, 40)
    with handle(2) as enc:
        enc.set_pcm_format(V.PCM_S16)
        rc, launches = bench.run(enc, [(0, 0, 0, 8)])
        assert rc == V.E_UNSUPPORTED and launches == [] and bench.untouched()
        enc.set_pcm_format(V.PCM_S32)
        assert bench.run(enc, [(0, 0, 0, 8)])[0] == V.OK and not bench.untouched()
