"""k_md5_ranges at the ABI level (fhip_md5_update_ranges_dev): every stream absorbs ranges of samples that device
tables name.  The witness is hashlib.md5 over the message built here in numpy, as in tests/test_gpu_md5_streams.py.

The shapes are the places where the kernel can go wrong: a stream that never completes a block, a range that ends exactly
on one, incoming fills of 1, 63, 2 and 3 bytes, ranges that start at odd sample indices (so that int16 data is only
2-byte aligned and int32 data only 4-byte), bodies that are no whole number of units, an empty range between two others,
streams without a range, 65 streams (two waves, the second nearly empty) and two updates in a row.  The last range of the
buffer is a long one that ends where the data ends; behind it lies a sentinel region, which a body that read one unit too
far would hash."""
import hashlib

import numpy as np
import pytest

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
SB = V.MD5_STATE_BYTES
S = 65
SENT_VALS = 512


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def message(vals, bits):
    nb = (bits + 7) // 8
    return np.ascontiguousarray(vals.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def plan(r, ch, nb, update):
    """Per stream the lengths (samples per channel) of its ranges in this update."""
    unit = 64 if nb == 3 else 64 // nb                      # values per unit
    block = 192 if nb == 3 else 64
    per = ch * nb                                           # message bytes per sample
    whole = 2 * block * per // np.gcd(block, per) // per    # samples that end exactly on a block, twice over
    whole = int(whole)
    out = [[int(x) for x in r.randint(0, 300, r.randint(1, 4))] for _ in range(S)]
    out[11] = [350]                                         # the longest: it is laid out last
    if update == 0:
        out[0] = [max(1, 40 // per)]                        # fewer than 64 bytes: no block completes
        out[1] = [whole]
        out[2] = [70, 0, 33]                                # an empty range between two others
        out[3] = []                                         # no range: the state must not change
        out[5], out[6], out[7], out[8] = [1], [63], [2], [3]        # at one byte per mono sample: fills 1, 63, 2, 3
        out[9] = [(3 * unit + 17 + ch - 1) // ch]           # a body of three units and a remainder
    else:
        out[0] = [max(1, 20 // per)]                        # still below one block (at most 60 bytes in all)
        out[1] = [whole, 5]
        out[10] = []
        out[64] = [2 * unit + 1]                            # the lane that is alone in its wave
    return out


@pytest.mark.parametrize("ch,bits,fmt", [(1, 8, V.PCM_S32), (2, 8, V.PCM_S16), (1, 16, V.PCM_S16), (2, 16, V.PCM_S16),
                                         (1, 12, V.PCM_S32), (2, 16, V.PCM_S32), (1, 24, V.PCM_S32), (2, 24, V.PCM_S32),
                                         (2, 20, V.PCM_S32), (1, 32, V.PCM_S32), (2, 32, V.PCM_S32), (1, 4, V.PCM_S16)])
def test_ranges_against_hashlib(torch, ch, bits, fmt):
    r = np.random.RandomState(ch * 1000 + bits * 10 + fmt)
    nb = (bits + 7) // 8
    dtype = np.int16 if fmt == V.PCM_S16 else np.int32
    tname = "int16_t" if fmt == V.PCM_S16 else "int32_t"
    dev = torch.device("cuda", 0)
    ref = [hashlib.md5() for _ in range(S)]
    nbytes = np.zeros(S, np.int64)
    with V.Encoder(V.level_params(5, channels=ch, bits_per_sample=bits), max_frames=4) as enc:
        enc.set_pcm_format(fmt)
        states = torch.zeros(S * SB, dtype=torch.uint8, device=dev)
        digests = torch.zeros(S * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        enc.md5_init_dev(states, S)
        enc.sync()
        for update in range(2):
            lens = plan(r, ch, nb, update)
            ranges = [(s, j) for s in range(S) for j in range(len(lens[s]))]
            order = [ranges[i] for i in r.permutation(len(ranges))]
            longest = max(ranges, key=lambda sj: lens[sj[0]][sj[1]])
            order.remove(longest)
            order.append(longest)                              # a long body ends where the data ends
            # lay the ranges out with gaps of one or three samples: every start is odd or even as it comes, the first is 1
            start, pos = {}, 1
            for s, j in order:
                start[(s, j)] = pos
                pos += lens[s][j] + (0 if (s, j) == longest else int(r.choice([1, 3])))
            end = pos
            assert start[longest] + lens[longest[0]][longest[1]] == end and lens[longest[0]][longest[1]] >= 300
            assert any(v % 2 for v in start.values())
            lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
            pcm = r.randint(lo, hi + 1, end * ch + SENT_VALS, dtype=np.int64).astype(dtype)
            sentinel = pcm[end * ch:].copy()
            rid = {sj: i for i, sj in enumerate(order)}
            r_start = np.array([start[sj] for sj in order] + [0], np.int64)
            r_len = np.array([lens[s][j] for s, j in order] + [0], np.int64)
            seg_first = np.zeros(S + 1, np.int32)
            seg_range = []
            for s in range(S):
                for j in range(len(lens[s])):
                    a = start[(s, j)] * ch
                    seg_range.append(rid[(s, j)])
                    ref[s].update(message(pcm[a:a + lens[s][j] * ch], bits))
                    nbytes[s] += lens[s][j] * ch * nb
                seg_first[s + 1] = len(seg_range)
            seg_range = np.asarray(seg_range + [0], np.int32)
            tens = [torch.from_numpy(a).to(dev) for a in (pcm, seg_first, seg_range, r_start, r_len)]
            before = states.cpu().numpy().copy()
            torch.cuda.synchronize()
            enc.md5_update_ranges_dev(states, S, *tens)
            assert enc.last_launches() == [f"k_md5_ranges<{tname},{nb}>"]
            enc.md5_final_dev(states, S, digests)
            enc.sync()
            after = states.cpu().numpy()
            got = digests.cpu().numpy().reshape(S, 16)
            for s in range(S):
                assert got[s].tobytes() == ref[s].digest(), (update, s, lens[s], [start[(s, j)] for j in range(len(lens[s]))])
            st = np.frombuffer(after.tobytes(), V.MD5_STATE_DTYPE)
            assert (st["nbytes"] == nbytes.astype(np.uint64)).all()
            assert (st["fill"] == (nbytes % 64).astype(np.uint32)).all()
            for s in range(S):
                if not lens[s]:
                    assert after[s * SB:(s + 1) * SB].tobytes() == before[s * SB:(s + 1) * SB].tobytes(), s
            assert np.array_equal(tens[0].cpu().numpy()[end * ch:], sentinel)      # nothing was written behind the data
        assert nbytes[0] < 64                                                       # the stream that never completed a block


def test_null_and_negative_arguments(torch):
    dev = torch.device("cuda", 0)
    with V.Encoder(V.level_params(5), max_frames=4) as enc:
        states = torch.zeros(2 * SB, dtype=torch.uint8, device=dev)
        z32 = torch.zeros(4, dtype=torch.int32, device=dev)
        z64 = torch.zeros(4, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        lib, h = enc.lib, enc._h
        p = V._ptr
        assert lib.fhip_md5_update_ranges_dev(h, None, 2, p(z32), p(z32), p(z32), p(z64), p(z64)) == V.E_INVALID
        assert lib.fhip_md5_update_ranges_dev(h, p(states), 2, p(z32), p(z32), p(z32), None, p(z64)) == V.E_INVALID
        assert lib.fhip_md5_update_ranges_dev(h, p(states), -1, p(z32), p(z32), p(z32), p(z64), p(z64)) == V.E_INVALID
        assert enc.last_launches() == []
        enc.md5_update_ranges_dev(states, 0, z32, z32, z32, z64, z64)              # no stream: nothing to do
        assert enc.last_launches() == []
