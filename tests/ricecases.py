"""Rice-parameter boundary cases: one table of frames whose partition sums sit exactly on the limits at which the
encoder's closed forms for find_optimal_rice_param (rice.c:30-45) change branch, and a plain restatement of
rice.c:30-139 and of the stereo estimate (encode.c:595-640) to say what each frame must give.  TEST INFRASTRUCTURE ONLY.

The construction.  A block whose only non-zero samples are impulses more than max_prediction_order apart has zero
windowed autocorrelation at lags 1 .. order: every coefficient row quantises to zeros with shift 0 and the LPC residual
behind the warm-up IS the sample; under the fixed predictor pinned to order 0 it is the sample outright, however dense.
A 32-bit sample folds ((2x) ^ (x >> 31)) to any value below 2^32, so every partition sum of every level can be set to
the integer a case asks for through the public entries.

The restatement is numpy and Python integers only; it shares no text with the device code or the C oracle.

Families (Case.family):
  F1  a node's sum against cnt >> 1: 0, half - 1, half, half + 1
  F2  S = sum - (cnt >> 1) against 2 cnt << k for every k the node can reach: (2cnt << k) - 1, 2cnt << k, (2cnt << k) + 1,
      ((2cnt + 1) << k) - 1, (2cnt + 1) << k -- the leading-zero estimate of k and its correction, both ways
  F3  the parameter at 14 | 15 (RICE | RICE2) in one partition of the finest level or of a coarser one, under a free
      partition-order search; the cap at 30
  F4  S and sum at 0xFFE00000 - 1, +0, +1 and sum at 2^32 - 1, +0, +1: in one level-6 node, in the block total alone
      (every level-6 node far below), in one level-8 node
  F5  thread sums: the largest folded value of a run on both sides of 2^(32 - ceil(log2 C)) in one wave (F5a); a run
      sum on both sides of 2^32 in one wave (F5b: two impulses inside one run of C samples)
  F6  the first partition: (n >> pmax) - order equal to 0 and to 1, a full-scale warm-up sample that must not count
  F7  a tie at the minimum between two partition orders (the higher wins, rice.c:131)
  F8  (K0) the left channel's 2 * sum of second differences at F1's and F2's limits and around 2^32

Sites (Case.site): S1 the workgroup-wide pyramid (k_encode_pow2<C,T,0>), S2 the one-wave search from 32-bit leaves
(<C,T,3> and <C,T,2>), S3 the fixed predictors' one-pass search and candidate loop (<C,T,1>), S4 the order search
(k_order_search, vector and matrix), S5 a variable-block-size batch, S6 K0's stereo estimate, S7 the baseline: the
generic search on given residuals (every case goes there as well) and a long block (k_encode_big).

EXCLUDED says which (site, family) pairs cannot exist, and why.
"""
from __future__ import annotations

import operator

import numpy as np

import flake_amd

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
THR = 0xFFE00000            # where the closed forms hand over to the scan
MAX_K = 30


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def fold(x: int) -> int:
    """rice.c:122 on an int32"""
    x = int(x)
    return ((2 * x) ^ (x >> 31)) & M32


def unfold(u: int) -> int:
    return (u >> 1) if not (u & 1) else -((u + 1) >> 1)


def fold_array(res) -> np.ndarray:
    x = np.asarray(res).astype(np.int64)
    return (((2 * x) ^ (x >> 31)) & M32).astype(np.uint64)


def log2i(v: int) -> int:
    return v.bit_length() - 1 if v > 0 else 0


def rice_count(s: int, n: int, k: int) -> int:
    """rice.h:48 as the macro evaluates it: n * (k + 1) an int, sum - (n >> 1) in uint64, a logical shift"""
    return (n * (k + 1) + (((s - (n >> 1)) & M64) >> k)) & M64


def scan_k(s: int, n: int, lt=operator.lt) -> int:
    """rice.c:30-45: the first strict minimum of the count truncated to uint32"""
    vals, kopt = [], 0
    for k in range(MAX_K + 1):
        vals.append(rice_count(s, n, k) & M32)
        if lt(vals[k], vals[kopt]):
            kopt = k
    return kopt


def closed_k(s: int, n: int, correction: bool = True) -> int:
    """The closed form the fast paths rely on, from its derivation: k = 0 below n >> 1; else the smallest k with
    (S >> k) <= 2n, capped at 30 -- a difference of bit lengths, corrected by one; the scan near 2^32 and for n <= 0."""
    half = n >> 1
    if s < half:
        return 0
    S = s - half
    if n <= 0 or S >= THR:
        return scan_k(s, n)
    two, k = 2 * n, 0
    if S > two:
        k = S.bit_length() - two.bit_length()
        if correction and (S >> k) > two:
            k += 1
        k = min(k, MAX_K)
    return k


def limit_porder(porder: int, n: int, order: int) -> int:
    """rice.c:148-155"""
    porder = min(porder, log2i(n ^ (n - 1)))
    if order > 0:
        porder = min(porder, log2i(n // order))
    return porder


def level_sums(res, order: int, pmin: int, pmax: int) -> dict:
    """rice.c:76-103 after the clamps: {level: [sums]}"""
    n = len(res)
    u = fold_array(res)
    cnt = n >> pmax
    sums = {pmax: [int(u[order:cnt].sum())] + [int(u[i * cnt:(i + 1) * cnt].sum()) for i in range(1, 1 << pmax)]}
    for p in range(pmax - 1, pmin - 1, -1):
        sums[p] = [sums[p + 1][2 * j] + sums[p + 1][2 * j + 1] for j in range(1 << p)]
    return sums


def calc_rice(res, order: int, pmin: int, pmax: int, lpc: bool, bps: int, precision: int,
              find_k=scan_k, le=operator.le) -> dict:
    """rice.c:47-187: bits, method, porder, params (and every level's bits, parameters and sums)"""
    n = len(res)
    pmin, pmax = limit_porder(pmin, n, order), limit_porder(pmax, n, order)
    sums = level_sums(res, order, pmin, pmax)
    lbits, lpar, lmeth = {}, {}, {}
    for p in range(pmin, pmax + 1):
        allb, ks = 0, []
        for i, s in enumerate(sums[p]):
            cnt = (n >> p) - (order if i == 0 else 0)
            k = find_k(s, cnt)
            ks.append(k)
            allb = (allb + rice_count(s, cnt, k)) & M32
        lbits[p], lpar[p], lmeth[p] = (allb + 4 * (1 << p)) & M32, ks, int(max(ks) > 14)
    opt = pmin
    for p in range(pmin + 1, pmax + 1):
        if le(lbits[p], lbits[opt]):
            opt = p
    bits = order * bps + 2
    if lpc:
        bits += 4 + 5 + order * precision
    bits = (bits + lbits[opt] + lmeth[opt] + 4) & M32
    return dict(bits=bits, method=lmeth[opt], porder=opt, params=lpar[opt], level_bits=lbits, level_params=lpar,
                level_method=lmeth, sums=sums, pmin=pmin, pmax=pmax)


def stereo_sums(left, right):
    """encode.c:607-616: the four sums of second differences (int32 arithmetic)"""
    def d2(x):
        x = np.asarray(x).astype(np.int64)
        t = x[2:] - 2 * x[1:-1] + x[:-2]
        return ((t + (1 << 31)) & M32) - (1 << 31)
    lt, rt = d2(left), d2(right)
    wrap = lambda v: ((v + (1 << 31)) & M32) - (1 << 31)
    return [int(np.abs(lt).sum()), int(np.abs(rt).sum()), int(np.abs(wrap(lt + rt) >> 1).sum()),
            int(np.abs(wrap(lt - rt)).sum())]


def stereo_mode(left, right, find_k=scan_k) -> int:
    """encode.c:598-643: 0 LEFT_RIGHT, 1 LEFT_SIDE, 2 RIGHT_SIDE, 3 MID_SIDE"""
    n = len(left)
    cost = []
    for s in stereo_sums(left, right):
        s2 = (2 * s) & M64
        cost.append(rice_count(s2, n, find_k(s2, n)))
    score = [(cost[0] + cost[1]) & M64, (cost[0] + cost[3]) & M64, (cost[1] + cost[3]) & M64, (cost[2] + cost[3]) & M64]
    best = 0
    for i in range(1, 4):
        if score[i] < score[best]:
            best = i
    return best


def clog2_up(c: int) -> int:
    return (c - 1).bit_length()


def thread_runs(res, order: int, C: int, T: int):
    """What a (C, T) geometry's threads hold: per wave, every thread's run sum and largest folded value (the warm-up
    zeroed).  Returns (sums[T / 64][64], maxes[T / 64][64]) as uint64."""
    u = fold_array(res).copy()
    u[:order] = 0
    assert len(u) == C * T
    r = u.reshape(T, C)
    w = max(T // 64, 1)
    return r.sum(axis=1).reshape(w, -1), r.max(axis=1).reshape(w, -1)


# ---------------------------------------------------------------------------------------------------------------------
# the sites
# ---------------------------------------------------------------------------------------------------------------------
class Cfg:
    """One instance of a site: block size, parameters, the geometry and launch it must take."""

    def __init__(self, site, n, C, T, launch, kw, ch=1, bps=32, order=None, entries=("encode",), search=None,
                 coarse_launch=None):
        self.site, self.n, self.C, self.T, self.launch, self.kw = site, n, C, T, launch, dict(kw)
        self.coarse_launch = coarse_launch          # the instance a smaller max_partition_order selects, if another
        self.ch, self.bps, self.entries, self.search = ch, bps, entries, search
        self.fixed = kw.get("prediction_type") == flake_amd.PRED_FIXED
        self.maxorder = 0 if self.fixed else kw["max_prediction_order"]
        # the order the encoder ends on: the pinned / maximum one, or (order searches over all-zero rows: the header
        # alone grows with the order) the lowest candidate -- asserted from the oracle's record
        self.order = self.maxorder if order is None else order
        self.spacing = self.maxorder + 1
        self.umax = (1 << bps) - 1
        self.pmax_req = kw["max_partition_order"]
        self.pf = limit_porder(self.pmax_req, n, self.order)          # the finest level the search reaches
        self.name = f"{site}-n{n}-{'fix' if self.fixed else 'o%d' % self.maxorder}-{ch}x{bps}-p{self.pmax_req}" + \
                    (f"-{search}" if search else "")

    def launch_for(self, pin=None):
        return self.launch if pin is None or pin == self.pf or self.coarse_launch is None else self.coarse_launch

    def params(self, pin=None):
        kw = dict(self.kw)
        kw.setdefault("min_partition_order", 0)
        if pin is not None:
            # (the finest level keeps the requested maximum, which clamps to it: the geometry can depend on the request)
            kw["min_partition_order"], kw["max_partition_order"] = pin, (self.pmax_req if pin == self.pf else pin)
        return flake_amd.level_params(5, channels=self.ch, bits_per_sample=self.bps, block_size=self.n, **kw)


def _lpc(order, pmax, om=None, lo=None):
    kw = dict(order_method=flake_amd.OM_MAX if om is None else om, max_prediction_order=order, max_partition_order=pmax)
    if lo is not None:
        kw["min_prediction_order"] = lo
    return kw


def _fixed0(pmax):
    return dict(prediction_type=flake_amd.PRED_FIXED, min_prediction_order=0, max_prediction_order=0,
                max_partition_order=pmax)


def site_configs():
    P = "k_encode_pow2<%d,%d,%d>"
    out = []
    # S1: the lean instance (one row, orders <= 8): the workgroup-wide pyramid
    for n, C, T, pmax in ((256, 4, 64, 6), (512, 8, 64, 6), (1024, 4, 256, 8), (2048, 8, 256, 8), (4096, 16, 256, 8),
                          (8192, 16, 512, 8), (16384, 16, 1024, 8), (1152, 9, 128, 8), (1536, 6, 256, 8)):
        out.append(Cfg("S1", n, C, T, P % (C, T, 0), _lpc(8, pmax)))
    for n, C, T in ((512, 8, 64), (2048, 8, 256), (4096, 16, 256)):
        out.append(Cfg("S1", n, C, T, P % (C, T, 0), _lpc(8, 6 if n == 512 else 8), ch=2, bps=16))
    # S2: the one-wave search from the thread sums: orders 9 .. 16 (MODE 3), several rows without a search kernel (MODE 2)
    for n, C, T, pmax in ((512, 2, 256, 7), (1024, 4, 256, 8), (2048, 8, 256, 8), (4096, 16, 256, 8), (8192, 16, 512, 8)):
        # (512 samples take runs of 2 only where partition orders 7, 8 are asked for; pinned lower they take (8,64))
        out.append(Cfg("S2", n, C, T, P % (C, T, 3), _lpc(12, pmax), coarse_launch=P % (8, 64, 3) if n == 512 else None))
    out.append(Cfg("S2", 2048, 8, 256, P % (8, 256, 3), _lpc(12, 8), ch=2, bps=16))
    out.append(Cfg("S2", 2304, 9, 256, P % (9, 256, 2), _lpc(8, 8, om=flake_amd.OM_4LEVEL, lo=1), order=2, search="4level"))
    # S3: fixed predictors, order pinned to 0: the one-pass search (partition orders <= 5) and the candidate loop
    for n, C, T in ((256, 4, 64), (1152, 9, 128), (4096, 16, 256)):
        for bps in (32, 16):
            out.append(Cfg("S3", n, C, T, P % (C, T, 1), _fixed0(5), bps=bps))
            out.append(Cfg("S3", n, C, T, P % (C, T, 1), _fixed0(6 if n == 256 else 8), bps=bps))
    # S4: the order-search kernel: a wave per candidate from the thread sums; the matrix search (24 bits)
    S = "k_order_search<%d,%d,4,%s>"
    both = ("encode", "table")
    for n, C, T in ((1024, 4, 256), (1536, 12, 128), (2560, 20, 128), (4096, 16, 256)):
        out.append(Cfg("S4", n, C, T, S % (C, T, "false"), _lpc(12, 8, om=flake_amd.OM_SEARCH, lo=1), order=1,
                       entries=both, search="search"))
    out.append(Cfg("S4", 4096, 16, 256, S % (16, 256, "true"), _lpc(12, 8, om=flake_amd.OM_SEARCH, lo=1), bps=24, order=1,
                   entries=both, search="search"))
    out.append(Cfg("S4", 4096, 16, 256, S % (16, 256, "false"), _lpc(12, 8, om=flake_amd.OM_8LEVEL, lo=3), order=3,
                   entries=both, search="8level"))
    out.append(Cfg("S4", 4096, 16, 256, S % (16, 256, "false"), _lpc(12, 8, om=flake_amd.OM_LOG, lo=1), order=None,
                   entries=both, search="log"))
    out.append(Cfg("S4", 1024, 4, 256, S % (4, 256, "false"), _lpc(32, 8, om=flake_amd.OM_SEARCH, lo=1), order=1,
                   entries=both, search="search32"))
    # S7: a long block (the streaming K3); every case's residuals also go through the generic search
    out.append(Cfg("S7", 16385, 0, 0, "k_encode_big", _lpc(8, 8)))
    return out


# F6's own instances: (n >> pmax) - order is 0 or 1 at the finest level the reference lets through
def first_partition_configs():
    P = "k_encode_pow2<%d,%d,%d>"
    return [Cfg("S1", 2048, 8, 256, P % (8, 256, 0), _lpc(8, 8)), Cfg("S1", 2048, 8, 256, P % (8, 256, 0), _lpc(7, 8)),
            Cfg("S1", 256, 4, 64, P % (4, 64, 0), _lpc(8, 6)), Cfg("S1", 256, 4, 64, P % (4, 64, 0), _lpc(7, 6)),
            Cfg("S2", 4096, 16, 256, P % (16, 256, 3), _lpc(16, 8)), Cfg("S2", 4096, 16, 256, P % (16, 256, 3), _lpc(15, 8)),
            Cfg("S2", 2048, 8, 256, P % (8, 256, 3), _lpc(16, 8)), Cfg("S2", 2048, 8, 256, P % (8, 256, 3), _lpc(15, 8))]


EXCLUDED = {
    ("S3", "F6"): "the fixed predictor is pinned to order 0: no warm-up, the first partition is never short",
    ("S4", "F6"): "the searches end on a low order of all-zero rows: (n >> 8) - order is never 0 or 1 there",
    ("S4", "F7"): "the tie heights hold for one known order; which order a search ends on is its own to decide",
    ("S7", "F4"): "the long block is 16385 samples: odd, so its only partition order is 0 and its total is one node "
                  "(the generic search itself takes every case of the table, F4 included, as given residuals)",
    ("S7", "F5a"): "the generic search has no per-thread width switch", ("S7", "F5b"): "as F5a",
    ("S7", "F6"): "as F4: one partition, n - order samples", ("S7", "F7"): "as F4: one partition order, nothing to tie",
    ("S5", "*"): "the splitter (vbs.c:36-83) cuts a block where the samples tell it to, so no piece is built around a chosen "
                 "sum: the batch test sends whole frames of the table through k_order_search_bins / k_encode_bins, holds the "
                 "stream to the oracle's and reads back which partition sums of the pieces the cut left on F2's limits",
    ("S6", "F1-F7"): "K0 has no partitions: its four sums are F8's",
}
# Narrower limits inside the pairs that do exist:
#   F5b needs two impulses inside one run of C samples, C > max order + 1: (16,T) at orders 8 and 12 and every fixed
#   geometry have it, (2..9,T) under LPC do not;
#   F3's cap at 30 and parameters above 27 need impulses closer than LPC orders 8 .. 12 allow: the fixed sites reach them;
#   16-bit frames reach no sum near 2^29: F3, F4, F5 are 32-bit (24-bit: the matrix search) only, F3 also dense 16-bit;
#   the order searches (S4) choose the order, so no target sits in the first partition's chain (level 0 included).


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, cfg, family, name, segs, prop, pin=None):
        self.cfg, self.family, self.site, self.pin, self.prop = cfg, family, cfg.site, pin, prop
        self.segs = segs                                   # (first sample, count, stride, folded value)
        self.name = f"{cfg.name}-{family}-{name}"

    def folded(self) -> np.ndarray:
        u = np.zeros(self.cfg.n, np.uint64)
        for pos, cnt, stride, val in self.segs:
            u[pos:pos + cnt * stride:stride] = val
        return u

    def samples(self) -> np.ndarray:
        u = self.folded().astype(np.int64)
        return np.where(u & 1, -((u + 1) >> 1), u >> 1).astype(np.int32)

    def pcm(self) -> np.ndarray:
        """[n][channels]: the samples on channel 0, silence beside them"""
        out = np.zeros((self.cfg.n, self.cfg.ch), np.int32)
        out[:, 0] = self.samples()
        return out

    def params(self):
        return self.cfg.params(self.pin)

    def key(self):
        return (self.cfg.name, self.pin)


class _Frame:
    """Impulses placed left to right, never closer than the configuration's spacing."""

    def __init__(self, cfg, start=None):
        self.cfg, self.segs, self.failed = cfg, [], set()
        self.next = cfg.maxorder if start is None else start        # the warm-up stays silent

    def slots(self, lo, hi):
        lo = max(lo, self.next)
        return lo, max(0, -(-(hi - lo) // self.cfg.spacing))

    def put(self, lo, hi, total) -> bool:
        """`total` into [lo, hi) on as few impulses as it needs; one of them odd as a sample where it can be arranged
        (no wasted bits: encode.c:560-592 would shift the block)"""
        if total == 0:
            return True
        sp, umax = self.cfg.spacing, self.cfg.umax
        lo, m = self.slots(lo, hi)                 # the first free sample of the range, how many impulses fit
        k = -(-total // umax)
        if k > m:
            return False
        base, r = divmod(total, k)
        vals = [base + 1] * r + [base] * (k - r)
        if not any(v % 4 in (1, 2) for v in vals) and k < m and total >= 2:
            vals[0] -= 1
            vals.append(1)
        pos = lo
        for v in vals:
            if v:
                self.segs.append((pos, 1, 1, v))
            pos += sp
        self.next = pos
        return True

    def dense(self, lo, hi, total) -> bool:
        """spacing 1 only: `total` spread evenly over the whole of [lo, hi)"""
        m = hi - lo
        if total > m * self.cfg.umax:
            return False
        base, r = divmod(total, m)
        if r:
            self.segs.append((lo, r, 1, base + 1))
        if base:
            self.segs.append((lo + r, m - r, 1, base))
        self.next = hi
        return True

    def at(self, pos, u):
        assert pos >= self.next, (pos, self.next)
        self.segs.append((pos, 1, 1, u))
        self.next = pos + self.cfg.spacing

    def any_odd(self):
        return any(v % 4 in (1, 2) for _, _, _, v in self.segs)


def _node_range(cfg, level, j):
    ln = cfg.n >> level
    return j * ln, (j + 1) * ln


def _build(cfg, targets, keep_clear=(), strict=True):
    """targets: [(lo, hi, total)] in rising order, disjoint; every finest partition outside them (and outside the
    keep_clear ranges) gets a filler of folded value 1.  None where a total does not fit."""
    fr = _Frame(cfg)
    ln = cfg.n >> cfg.pf
    targets = sorted(targets)
    ti = 0
    for q in range(1 << cfg.pf):
        a, b = q * ln, (q + 1) * ln
        while ti < len(targets) and targets[ti][0] < b and targets[ti][0] >= a:
            lo, hi, total = targets[ti]
            ti += 1
            big = cfg.spacing == 1 and total > cfg.umax
            if not (fr.dense(lo, hi, total) if big else fr.put(lo, hi, total)):
                if strict:
                    return None
                fr.failed.add(lo)                  # (the impulses before it left too little room: the node stays empty)
        if any(lo < b and a < hi for lo, hi, _ in targets) or any(lo < b and a < hi for lo, hi in keep_clear):
            continue
        fr.put(a, b, 1)
    return fr if fr.any_odd() else None


def _cnt(cfg, level, j):
    return (cfg.n >> level) - (cfg.order if j == 0 else 0)


def _f2_values(cnt, k):
    two = 2 * cnt
    return [((two << k) - 1, "lo"), (two << k, "at"), ((two << k) + 1, "hi"), (((two + 1) << k) - 1, "c-"),
            ((two + 1) << k, "c+")]


def _capacity(cfg, level, j):
    lo, hi = _node_range(cfg, level, j)
    lo = max(lo, cfg.maxorder)
    return max(0, -(-(hi - lo) // cfg.spacing)) * cfg.umax


def _pinned_frames(cfg, family, level, wanted, label):
    """wanted: [(total, tag)] for nodes of `level`, packed into frames pinned to that level: nodes 1 .. 2^level - 2 (node 0
    as well where the order is certain), the last one left to a filler"""
    out = []
    nodes = 1 << level
    order_certain = cfg.search is None
    usable = list(range(0 if order_certain else 1, max(nodes - 1, 1)))
    if not usable:
        return out
    todo = list(wanted)
    fi = 0
    while todo:
        targets, named = [], []
        for j in usable:
            if not todo:
                break
            mk, tag = todo.pop(0)
            cnt = _cnt(cfg, level, j)
            total = mk(cnt)
            if total is None or total < 0 or total > _capacity(cfg, level, j):
                continue
            lo, hi = _node_range(cfg, level, j)
            targets.append((lo, hi, total))
            named.append(dict(level=level, node=j, sum=total, cnt=cnt, tag=tag))
        if not targets:
            continue
        fr = _build(cfg, targets, strict=False)
        if fr is not None:
            named = [nd for nd, (lo, _, _) in zip(named, targets) if lo not in fr.failed]
            out.append(Case(cfg, family, f"{label}-L{level}-{fi}", fr.segs, dict(nodes=named), pin=level))
        fi += 1
    return out


def _levels_for(cfg):
    return sorted({cfg.pf, min(6, cfg.pf), min(3, cfg.pf), 0})


def family_f1_f2(cfg):
    out = []
    for level in _levels_for(cfg):
        f1 = [((lambda cnt, d=d: 0 if d is None else (cnt >> 1) + d), f"half{d}") for d in (None, -1, 0, 1)]
        out += _pinned_frames(cfg, "F1", level, f1, "half")
        ks = range(MAX_K + 1) if level else (0, 1, 8, 14, 15, 20, 24, 26, 27, 28, 29, 30)
        f2 = []
        for k in ks:
            for i in range(5):
                f2.append(((lambda cnt, k=k, i=i: _f2_values(cnt, k)[i][0] + (cnt >> 1)), f"k{k}{_f2_values(1, k)[i][1]}"))
        out += _pinned_frames(cfg, "F2", level, f2, "shift")
    return out


def family_f3(cfg):
    """k at 14 | 15 in one partition under a free partition-order search, and the cap at 30"""
    out = []
    for level in sorted({cfg.pf, min(5, cfg.pf), max(cfg.pf - 2, 0)}):
        nodes = 1 << level
        j = min(nodes - 1, max(1, nodes // 2 + 1)) if nodes > 1 else 0
        if j == 0 and cfg.search is not None:
            continue
        cnt = _cnt(cfg, level, j)
        two = 2 * cnt
        for S, tag in ((((two + 1) << 14) - 1, "k14"), ((two + 1) << 14, "k15"), (two << 15, "k15top"), ((two << 15) + 1, "k16"),
                       (((two + 1) << 29) - 1, "k29"), ((two + 1) << 29, "k30"), ((two + 1) << 31, "cap30")):
            total = S + (cnt >> 1)
            if total > _capacity(cfg, level, j):
                continue
            lo, hi = _node_range(cfg, level, j)
            fr = _build(cfg, [(lo, hi, total)])
            if fr is not None:
                out.append(Case(cfg, "F3", f"{tag}-L{level}", fr.segs,
                                dict(nodes=[dict(level=level, node=j, sum=total, cnt=cnt, tag=tag)])))
    return out


def family_f4(cfg):
    """sums and S around 0xFFE00000 and 2^32, free search and pinned to the node's level"""
    out = []
    if cfg.bps != 32:
        return out
    places = []
    if cfg.pf >= 6:
        places.append(("l6", 6, 37))
    if cfg.pf >= 8:
        places.append(("l8", 8, 150))
    if cfg.pf < 6 and cfg.pf >= 1:
        places.append((f"l{cfg.pf}", cfg.pf, (1 << cfg.pf) - 3 if cfg.pf > 1 else 1))
    for place, level, j in places:
        cnt = _cnt(cfg, level, j)
        half = cnt >> 1
        for total, tag in [(THR + d + half, f"S{d:+d}") for d in (-1, 0, 1)] + [(THR + d, f"sum{d:+d}") for d in (-1, 0, 1)] + \
                          [((1 << 32) + d, f"two32{d:+d}") for d in (-1, 0, 1)]:
            if total > _capacity(cfg, level, j):
                continue
            lo, hi = _node_range(cfg, level, j)
            fr = _build(cfg, [(lo, hi, total)])
            if fr is None:
                continue
            for pin in (None, level):
                out.append(Case(cfg, "F4", f"{place}-{tag}-{'free' if pin is None else 'pin'}", fr.segs,
                                dict(nodes=[dict(level=level, node=j, sum=total, cnt=cnt, tag=tag)], place=place), pin=pin))
    # the block total alone: spread over the nodes of level min(6, pf), each far below the threshold
    if cfg.search is None and cfg.pf >= 2:
        lv = min(6, cfg.pf)
        parts = 1 << lv
        cnt = _cnt(cfg, 0, 0)
        half = cnt >> 1
        for total, tag in [(THR + d + half, f"S{d:+d}") for d in (-1, 0, 1)] + [(THR + d, f"sum{d:+d}") for d in (-1, 0, 1)] + \
                          [((1 << 32) + d, f"two32{d:+d}") for d in (-1, 0, 1)]:
            base, r = divmod(total, parts)
            targets = []
            for q in range(parts):
                lo, hi = _node_range(cfg, lv, q)
                targets.append((lo, hi, base + (1 if q < r else 0)))
            fr = _build(cfg, targets)
            if fr is None:
                continue
            for pin in (None, 0):
                out.append(Case(cfg, "F4", f"total-{tag}-{'free' if pin is None else 'pin'}", fr.segs,
                                dict(nodes=[dict(level=0, node=0, sum=total, cnt=cnt, tag=tag)], place="total",
                                     below=dict(level=lv, limit=THR)), pin=pin))
    return out


def family_f5(cfg):
    """the width switches of the thread sums, in one wave that is not wave 0 (the only wave where T = 64)"""
    out = []
    if cfg.bps != 32 or cfg.C == 0:
        return out
    C, T, sp = cfg.C, cfg.T, cfg.spacing
    wave = 1 if T > 64 else 0
    t = 64 * wave + 5
    thr = 1 << (32 - clog2_up(C))
    ln = cfg.n >> cfg.pf
    for d in (-1, 0, 1):
        pos = t * C + min(1, C - 1)
        fr = _build(cfg, [(pos, pos + 1, thr + d)], keep_clear=[(pos - sp - ln, pos + sp)])
        if fr is not None:
            out.append(Case(cfg, "F5a", f"umax{d:+d}", fr.segs,
                            dict(threads=dict(kind="umax", wave=wave, limit=thr, crosses=d >= 0, value=thr + d))))
    if C > sp:
        for d in (-1, 0, 1):
            pos = t * C
            fr = _Frame(cfg)
            for q in range(1 << cfg.pf):
                a, b = q * ln, (q + 1) * ln
                if a <= pos < b:
                    fr.at(pos, 1 << 31)
                    fr.at(pos + sp, (1 << 31) + d)
                if b <= pos - sp - ln or a >= pos + C + sp:
                    fr.put(a, b, 1)
            if fr.any_odd():
                out.append(Case(cfg, "F5b", f"runsum{d:+d}", fr.segs,
                                dict(threads=dict(kind="runsum", wave=wave, limit=1 << 32, crosses=d >= 0,
                                                  value=(1 << 32) + d))))
    return out


def family_f6(cfg):
    """the first partition of the finest level holds 0 or 1 residual; a full-scale sample in the warm-up"""
    out = []
    first = (cfg.n >> cfg.pf) - cfg.order
    assert first in (0, 1), (cfg.name, first)
    ln = cfg.n >> cfg.pf
    for warm, wtag in ((0, "quiet"), (M32, "loudwarm")):
        for v, tag in ((0, "zero"), (1, "one"), (M32, "full")):
            if first == 0 and v:
                continue
            fr = _Frame(cfg, start=0)
            if warm:
                fr.at(0, warm)                      # sample -2^31 at position 0: inside every order's warm-up
            if first == 1 and v:
                if warm and cfg.order < cfg.spacing:
                    continue                        # the one residual of partition 0 is closer than the spacing allows
                fr.at(cfg.order, v)
            for q in range(1, 1 << cfg.pf):
                fr.put(q * ln, (q + 1) * ln, 1 + (q % 5) * 77)
            if fr.any_odd():
                out.append(Case(cfg, "F6", f"first{first}-{wtag}-{tag}", fr.segs,
                                dict(first=first, nodes=[dict(level=cfg.pf, node=0, sum=v, cnt=first, tag=tag)])))
    return out


# F7: the first odd height (below 4001) of one impulse at sample order + 20, all else zero, at which two partition
# orders tie at the minimum -- found with the restatement, asserted again whenever the table is built.  (An even height
# would be shifted out as a wasted bit.)  Block sizes without an entry have no such height: 1024, 4096 and 16384 at
# order 8, 4096 at order 12, 1152 and 1536 at order 8, and the fixed predictor at partition orders <= 5 above n = 256.
TIE_HEIGHTS = {(256, 8, 6): 163, (512, 8, 6): 2503, (2048, 8, 8): 171, (8192, 8, 8): 747, (512, 12, 7): 201,
               (1024, 12, 8): 199, (2048, 12, 8): 165, (8192, 12, 8): 713, (256, "fix", 5): 65, (256, "fix", 6): 65,
               (1152, "fix", 8): 1833, (4096, "fix", 8): 269}


def family_f7(cfg):
    """a tie at the minimum between two partition orders: the higher must win"""
    a = TIE_HEIGHTS.get((cfg.n, "fix" if cfg.fixed else cfg.maxorder, cfg.pmax_req))
    if cfg.search is not None or a is None:
        return []
    pos = cfg.maxorder + 20
    res = np.zeros(cfg.n, np.int32)
    res[pos] = a
    hi = calc_rice(res, cfg.order, 0, cfg.pmax_req, not cfg.fixed, cfg.bps, 15)
    lo = calc_rice(res, cfg.order, 0, cfg.pmax_req, not cfg.fixed, cfg.bps, 15, le=operator.lt)
    assert hi["porder"] > lo["porder"] and hi["level_bits"][hi["porder"]] == lo["level_bits"][lo["porder"]], cfg.name
    assert hi["level_bits"][hi["porder"]] == min(hi["level_bits"].values()), cfg.name
    return [Case(cfg, "F7", f"tie-a{a}", [(pos, 1, 1, fold(a))],
                 dict(tie=dict(height=a, levels=(lo["porder"], hi["porder"]), bits=hi["level_bits"][hi["porder"]])))]


_CASES = None


def cases():
    """The whole table (built once)."""
    global _CASES
    if _CASES is None:
        out = []
        for cfg in site_configs():
            out += family_f1_f2(cfg) + family_f3(cfg) + family_f4(cfg) + family_f5(cfg) + family_f7(cfg)
        for cfg in first_partition_configs():
            out += family_f6(cfg)
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        _CASES = out
    return _CASES


def groups():
    """{(configuration name, pinned level): [cases]}: the cases that share one parameter set, hence one call"""
    g = {}
    for c in cases():
        g.setdefault(c.key(), []).append(c)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# F8: K0's stereo estimate
# ---------------------------------------------------------------------------------------------------------------------
class StereoCase:
    def __init__(self, n, bps, name, left, right, prop):
        self.n, self.bps, self.name, self.left, self.right, self.prop = n, bps, name, left, right, prop
        self.family, self.site = "F8", "S6"

    def pcm(self):
        return np.stack([self.left, self.right], 1).astype(np.int32)


def _second_diff_channel(n, total, amp):
    """A channel whose sum of |x[i] - 2 x[i-1] + x[i-2]| over i >= 2 is `total`: impulses (4 |a| each) five samples
    apart, one step (2 |h|), and an initial slope of 1 ended at i = 2 (adds 1).  None if it does not fit."""
    x = np.zeros(n, np.int64)
    rest = total
    if rest & 1:
        x[1], x[2:] = 1, 2
        rest -= 1
    pos = 8
    while rest >= 4:
        if pos + 4 >= n - 8:
            return None
        a = min(rest // 4, amp)
        x[pos] += a
        rest -= 4 * a
        pos += 5
    if rest == 2:
        x[n - 4:] += 1
        rest = 0
    assert rest == 0
    return x


def stereo_cases(shapes=((256, 16), (256, 32), (4096, 16), (4096, 32))):
    out = []
    for n, bps in shapes:
        amp = (1 << (bps - 3)) - 1                    # 2a and the second difference stay inside the sample width
        half = n >> 1
        sums = [(0, "zero"), ((half - 2) // 2, "half-"), (half // 2, "half"), ((half + 2) // 2, "half+")]
        for k in (0, 1, 8, 20):
            for v, tag in _f2_values(n, k):
                s2 = v + half                        # 2 * sum wanted
                sums.append(((s2 + 1) // 2, f"k{k}{tag}"))
        if bps == 32:
            sums += [((1 << 31) + d, f"two32{2 * d:+d}") for d in (-1, 0, 1)]
        for i, (sm, tag) in enumerate(sums):
            left = _second_diff_channel(n, sm, amp)
            if left is None:
                continue
            for rname, right in (("silent", np.zeros(n, np.int64)), ("same", left.copy()),
                                 ("near", _second_diff_channel(n, max(sm - 3 + (i % 7), 0), amp))):
                if right is None:
                    continue
                out.append(StereoCase(n, bps, f"S6-n{n}-{bps}-{tag}-{rname}", left, right,
                                      dict(left_sum=sm, two_sum=2 * sm, n=n, tag=tag)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what the tests share: the oracle's answer per group (computed once), the reference's recorded answers
# ---------------------------------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(oracle, key):
    """(params, pcm[cases][n][ch], the oracle's batch) of one group; cached, never modified by the tests"""
    if key not in _EXPECTED:
        lst = groups()[key]
        p, n = lst[0].params(), lst[0].cfg.n
        pcm = np.stack([c.pcm() for c in lst])
        exp = oracle.encode_subframes_batch(p, pcm, n, slot_bytes=flake_amd.rice_slot_bytes(p, n))
        for a in exp.values():
            a.setflags(write=False)
        _EXPECTED[key] = (p, pcm, exp)
    return _EXPECTED[key]


def records(oracle):
    """[(case, params, channel 0's record, channel 0's residual)] over the whole table"""
    out = []
    for key, lst in groups().items():
        p, _, exp = expected(oracle, key)
        for i, c in enumerate(lst):
            out.append((c, p, exp["info"][i * p.channels], exp["residual"][i, 0]))
    return out


def rice_call(p, info):
    """the arguments of calc_rice_params_lpc / _fixed (rice.c:173-187) behind a record: (lpc, pmin, pmax, order, bps, precision)"""
    return (int(info["type"]) == 32, p.min_partition_order, p.max_partition_order, int(info["order"]), int(info["obits"]),
            p.lpc_precision)


def pack_answers(answers):
    """{name: (bits, method, porder, params)} as arrays (results only)"""
    names = sorted(answers)
    par = [np.asarray(answers[k][3][:1 << answers[k][2]], np.uint8) for k in names]
    return dict(names=np.array(names), bits=np.array([answers[k][0] for k in names], np.uint32),
                method=np.array([answers[k][1] for k in names], np.uint8),
                porder=np.array([answers[k][2] for k in names], np.uint8),
                params=np.concatenate(par), params_len=np.array([len(a) for a in par], np.uint32))


def unpack_answers(z):
    offs = np.concatenate([[0], np.cumsum(z["params_len"], dtype=np.int64)]).tolist()
    names, bits, meth, por, par = (z[k].tolist() for k in ("names", "bits", "method", "porder", "params"))
    return {names[i]: (bits[i], meth[i], por[i], par[offs[i]:offs[i + 1]]) for i in range(len(names))}
