"""K6 at the ABI level (fhip_md5_init_dev / _update_dev / _final_dev on device tensors): the MD5 of many streams,
one lane per stream.

The witness is hashlib.md5 over the message built here in numpy: for every interleaved sample the low
(bits_per_sample + 7) / 8 bytes of its value, little-endian -- what md5.c:281-320 feeds the hash.  Which path a
launch took is read from fhip_last_launches and held to what the shapes and the byte counts kept here require:
"fast" exactly when the block is a whole number of 64-byte MD5 blocks and no stream of the call holds a partial one."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import flake_amd
from cases import _rng

pytestmark = pytest.mark.gpu

V = flake_amd
SB = V.MD5_STATE_BYTES


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("no HIP device")
    return t


def message(vals, bits):
    """The bytes the hash sees for interleaved sample values (any integer dtype)."""
    nb = (bits + 7) // 8
    return np.ascontiguousarray(vals.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def random_pcm(r, nvals, bits, dtype):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return r.randint(lo, hi + 1, nvals, dtype=np.int64).astype(dtype)


class Streams:
    """nstreams running hashes on the device and their hashlib twins."""

    def __init__(self, torch, ch, bits, fmt, nstreams):
        self.t, self.dev = torch, torch.device("cuda", 0)
        self.ch, self.bits, self.fmt, self.S = ch, bits, fmt, nstreams
        self.nb = (bits + 7) // 8
        self.dtype = np.int16 if fmt == V.PCM_S16 else np.int32
        self.enc = V.Encoder(V.level_params(5, channels=ch, bits_per_sample=bits), max_frames=4)
        self.enc.set_pcm_format(fmt)
        self.states = torch.zeros(nstreams * SB, dtype=torch.uint8, device=self.dev)
        self.digests = torch.zeros(nstreams * 16, dtype=torch.uint8, device=self.dev)
        self.ref = [hashlib.md5() for _ in range(nstreams)]
        self.nbytes = np.zeros(nstreams, np.int64)
        torch.cuda.synchronize()
        self.enc.md5_init_dev(self.states, nstreams)
        self.keep = []

    def close(self):
        self.enc.sync()
        self.enc.close()

    def update(self, r, n, counts, order):
        """One launch: stream s gets counts[s] blocks of n samples; order: "rr" lays the blocks out round-robin in
        the PCM buffer, "random" in a seeded permutation.  Returns the launch list."""
        pairs = [(j, s) for s in range(self.S) for j in range(counts[s])]
        pairs.sort()                                           # round-robin: all first blocks, all second ...
        if order == "random":
            pairs = [pairs[i] for i in r.permutation(len(pairs))]
        nblocks = max(len(pairs), 1)
        bv = n * self.ch
        pcm = random_pcm(r, nblocks * bv, self.bits, self.dtype).reshape(nblocks, bv)
        where = {}
        for slot, (j, s) in enumerate(pairs):
            where[(s, j)] = slot
        seg_first = np.zeros(self.S + 1, np.int32)
        seg_block = []
        all_aligned = bool((self.nbytes % 64 == 0).all())
        for s in range(self.S):
            for j in range(counts[s]):
                seg_block.append(where[(s, j)])
                self.ref[s].update(message(pcm[where[(s, j)]], self.bits))
                self.nbytes[s] += bv * self.nb
            seg_first[s + 1] = len(seg_block)
        seg_block = np.asarray(seg_block + [0], np.int32)
        t = self.t
        pcm_t, sf_t, sb_t = (t.from_numpy(a).to(self.dev) for a in (pcm, seg_first, seg_block))
        self.keep = [pcm_t, sf_t, sb_t]
        t.cuda.synchronize()
        self.enc.md5_update_dev(self.states, self.S, pcm_t, n, sf_t, sb_t)
        launches = self.enc.last_launches()
        want = "fast" if (bv * self.nb) % 64 == 0 and all_aligned else "general"
        tname = "int16_t" if self.fmt == V.PCM_S16 else "int32_t"
        assert launches[-1] == f"k_md5_streams<{tname},{self.nb}> {want}", (launches, n, self.ch, self.bits)
        return launches

    def raw_states(self):
        self.enc.sync()
        return self.states.cpu().numpy().copy()

    def check(self, what=""):
        self.enc.md5_final_dev(self.states, self.S, self.digests)
        self.enc.sync()
        got = self.digests.cpu().numpy().reshape(self.S, 16)
        for s in range(self.S):
            assert got[s].tobytes() == self.ref[s].digest(), (what, s, self.ch, self.bits, self.fmt)
        st = np.frombuffer(self.raw_states().tobytes(), V.MD5_STATE_DTYPE)
        assert (st["nbytes"] == self.nbytes.astype(np.uint64)).all()
        assert (st["fill"] == (self.nbytes % 64).astype(np.uint32)).all()
        return got


MATRIX = [(ch, bits, V.PCM_S32) for ch in (1, 2, 3, 8) for bits in (8, 12, 16, 20, 24, 32)] + \
         [(ch, bits, V.PCM_S16) for ch in (1, 2, 3, 8) for bits in (8, 12, 16)]


@pytest.mark.parametrize("nstreams", (1, 3, 64, 65, 1000))
@pytest.mark.parametrize("ch,bits,fmt", MATRIX)
def test_digests_equal_hashlib(torch, ch, bits, fmt, nstreams):
    """States carried over five launches: two fast-shaped ones (192 samples: a whole number of 64-byte blocks at
    every channel count and width), a short odd one, and two more fast-shaped ones that must run general where the
    odd one left partial blocks.  Streams get 0..3 blocks per launch; the layouts alternate."""
    r = _rng(1000 * ch + 10 * bits + fmt + 7 * nstreams)
    st = Streams(torch, ch, bits, fmt, nstreams)
    try:
        for k, n in enumerate((192, 192, 21, 192, 64)):
            counts = r.randint(0, 4, nstreams)
            if nstreams > 1 and k != 2:
                counts[r.randint(0, nstreams)] = 0             # somebody always sits a launch out
            if k == 0:
                counts[0] = max(counts[0], 1)
            st.update(r, n, counts, "rr" if k % 2 == 0 else "random")
            if k in (1, 4):
                st.check(f"after launch {k}")
    finally:
        st.close()


@pytest.mark.parametrize("n", (4096, 1152, 4608))
@pytest.mark.parametrize("ch,bits,fmt", [(2, 16, V.PCM_S16), (2, 16, V.PCM_S32), (2, 24, V.PCM_S32), (8, 24, V.PCM_S32),
                                         (1, 8, V.PCM_S32), (2, 8, V.PCM_S16), (2, 32, V.PCM_S32)])
def test_preset_block_sizes_take_the_fast_path(torch, ch, bits, fmt, n):
    r = _rng(n + ch + bits)
    st = Streams(torch, ch, bits, fmt, 70)
    try:
        for k in range(3):
            launches = st.update(r, n, r.randint(0, 3, 70), "random")
            assert launches[-1].endswith(" fast"), launches
            assert launches[0] == "k_md5_scan", launches
        st.check()
    finally:
        st.close()


@pytest.mark.parametrize("ch,bits,n,fill", [(1, 8, 1000, 40), (2, 24, 16, 32)])
def test_general_path_and_a_fast_shape_behind_it(torch, ch, bits, n, fill):
    """1000 mono 8-bit samples leave 40 bytes waiting, 16 stereo 24-bit ones (96 bytes) 32: both launches are general
    by shape, and the 4096-sample launch behind them is general because fill != 0 -- until a second odd block has
    made the streams whole again."""
    r = _rng(n)
    S = 67
    st = Streams(torch, ch, bits, V.PCM_S32, S)
    try:
        ones = np.ones(S, np.int64)
        assert st.update(r, n, ones, "rr")[-1].endswith(" general")
        assert (st.nbytes % 64 == fill).all()
        st.check("odd")
        assert st.update(r, 4096, ones, "random")[-1].endswith(" general")
        st.check("fast shape on partial blocks")
        # bring every stream back to a multiple of 64 bytes, then the same shape runs fast
        bv = ch * ((bits + 7) // 8)
        back = next(m for m in range(1, 65) if (fill + m * bv) % 64 == 0 and (m * bv) % 64 != 0)
        assert st.update(r, back, ones, "rr")[-1].endswith(" general")
        assert st.update(r, 4096, ones, "random")[-1].endswith(" fast")
        st.check("whole again")
    finally:
        st.close()


def test_untouched_stream_keeps_its_state_bit_for_bit(torch):
    r = _rng(5)
    S = 130
    st = Streams(torch, 2, 16, V.PCM_S16, S)
    try:
        st.update(r, 1152, np.full(S, 2), "rr")
        st.update(r, 100, np.full(S, 1), "rr")                  # partial blocks everywhere
        before = st.raw_states().reshape(S, SB)
        for n in (1152, 100):                                   # the general path both times (fill != 0), two shapes
            counts = np.zeros(S, np.int64)
            counts[1::2] = 1
            st.update(r, n, counts, "random")
        after = st.raw_states().reshape(S, SB)
        assert (after[0::2] == before[0::2]).all()
        assert (after[1::2] != before[1::2]).any(axis=1).all()
        st.check()
        # and on the fast path
        st2 = Streams(torch, 2, 16, V.PCM_S16, S)
        try:
            st2.update(r, 1152, np.full(S, 1), "rr")
            b2 = st2.raw_states().reshape(S, SB)
            counts = np.zeros(S, np.int64)
            counts[::3] = 2
            assert st2.update(r, 4096, counts, "random")[-1].endswith(" fast")
            a2 = st2.raw_states().reshape(S, SB)
            keep = np.ones(S, bool)
            keep[::3] = False
            assert (a2[keep] == b2[keep]).all()
            st2.check()
        finally:
            st2.close()
    finally:
        st.close()


def test_final_leaves_the_states_usable(torch):
    r = _rng(6)
    S = 9
    st = Streams(torch, 2, 24, V.PCM_S32, S)
    try:
        st.check("empty message")                               # d41d8cd9...
        assert st.ref[0].hexdigest() == "d41d8cd98f00b204e9800998ecf8427e"
        st.update(r, 1000, np.full(S, 1), "rr")
        before = st.raw_states()
        a = st.check("first").copy()
        b = st.check("second").copy()
        assert (a == b).all()
        assert (st.raw_states() == before).all()                # final works on a copy
        st.update(r, 59, np.arange(S) % 3, "random")            # fills past 56: the length takes a block of its own
        st.update(r, 1, np.full(S, 1), "random")
        st.check("continued")
    finally:
        st.close()


def test_refusals_return_their_codes_and_launch_nothing(torch):
    dev = torch.device("cuda", 0)
    lib = V.load_library()
    with V.Encoder(V.level_params(5), max_frames=4) as enc:
        S = 4
        states = torch.zeros(S * SB, dtype=torch.uint8, device=dev)
        pcm = torch.zeros(4096 * 2, dtype=torch.int32, device=dev)
        sf = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        sb = torch.zeros(1, dtype=torch.int32, device=dev)
        dg = torch.zeros(S * 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        enc.md5_init_dev(states, S)
        enc.sync()
        mark = enc.last_launches()
        assert mark == ["k_md5_init"]
        before = states.cpu().numpy().copy()
        h, p = enc._h, V._ptr
        bad = [
            lib.fhip_md5_init_dev(h, None, S), lib.fhip_md5_init_dev(h, p(states), -1),
            lib.fhip_md5_init_dev(None, p(states), S),
            lib.fhip_md5_update_dev(h, None, S, p(pcm), 4096, p(sf), p(sb)),
            lib.fhip_md5_update_dev(h, p(states), S, None, 4096, p(sf), p(sb)),
            lib.fhip_md5_update_dev(h, p(states), S, p(pcm), 4096, None, p(sb)),
            lib.fhip_md5_update_dev(h, p(states), S, p(pcm), 4096, p(sf), None),
            lib.fhip_md5_update_dev(h, p(states), -2, p(pcm), 4096, p(sf), p(sb)),
            lib.fhip_md5_update_dev(h, p(states), S, p(pcm), 0, p(sf), p(sb)),
            lib.fhip_md5_update_dev(h, p(states), S, p(pcm), V.MAX_BLOCK + 1, p(sf), p(sb)),
            lib.fhip_md5_final_dev(h, None, S, p(dg)), lib.fhip_md5_final_dev(h, p(states), S, None),
            lib.fhip_md5_final_dev(h, p(states), -1, p(dg)),
            lib.fhip_md5_final(h, p(states), S, None),
            # no upload is pending on this handle
            lib.fhip_md5_update_uploaded(h, p(states), S, 1, 4096, np.zeros(S + 1, np.int32).ctypes.data,
                                         np.zeros(1, np.int32).ctypes.data),
        ]
        assert bad == [V.E_INVALID] * len(bad), bad
        assert enc.last_launches() == mark
        enc.sync()
        assert (states.cpu().numpy() == before).all()


def test_update_uploaded_hashes_the_packed_upload(torch):
    """fhip_md5_update_uploaded: host tables, the PCM of the handle's last fhip_frames_packed_upload; refused once
    fhip_frames_packed_begin has consumed the upload, and for tables that point outside it."""
    dev = torch.device("cuda", 0)
    lib = V.load_library()
    p = V.level_params(5)
    n, nb, S = p.block_size, 12, 5
    pcm = np.ascontiguousarray(V.synth_pcm(nb, n, 2, 16).astype(np.int16))
    with V.Encoder(p, max_frames=nb) as enc:
        enc.set_pcm_format(V.PCM_S16)
        states = torch.zeros(S * SB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        enc.md5_init_dev(states, S)
        fbytes = np.zeros(nb, np.int32)
        b = V.Batch(pcm.ctypes.data, nb, n, None, None, None, 0, None, None, None, 0, fbytes.ctypes.data, 0, None)
        sob = np.arange(nb) % S
        order = np.argsort(sob, kind="stable").astype(np.int32)
        first = np.concatenate([[0], np.cumsum(np.bincount(sob, minlength=S))]).astype(np.int32)
        assert lib.fhip_frames_packed_upload(enc._h, C.byref(b)) == V.OK
        outside = order.copy()
        outside[3] = nb
        assert lib.fhip_md5_update_uploaded(enc._h, V._ptr(states), S, nb, n, first.ctypes.data,
                                            outside.ctypes.data) == V.E_INVALID
        assert lib.fhip_md5_update_uploaded(enc._h, V._ptr(states), S, nb - 1, n, first.ctypes.data,
                                            order.ctypes.data) == V.E_INVALID
        assert lib.fhip_md5_update_uploaded(enc._h, V._ptr(states), S, nb, n, first.ctypes.data,
                                            order.ctypes.data) == V.OK
        assert enc.last_launches()[-1] == "k_md5_streams<int16_t,2> fast"
        total = C.c_int64(0)
        assert lib.fhip_frames_packed_begin(enc._h, C.byref(b), C.byref(total)) == V.OK
        assert total.value > 0 and (fbytes > 0).all()
        assert lib.fhip_md5_update_uploaded(enc._h, V._ptr(states), S, nb, n, first.ctypes.data,
                                            order.ctypes.data) == V.E_INVALID
        dg = np.zeros((S, 16), np.uint8)
        assert lib.fhip_md5_final(enc._h, V._ptr(states), S, dg.ctypes.data) == V.OK
        for s in range(S):
            assert dg[s].tobytes() == hashlib.md5(pcm[sob == s].tobytes()).digest(), s
