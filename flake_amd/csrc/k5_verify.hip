// k5_verify.hip -- K5: does every frame of a stream decode to the caller's PCM?
//
// The verifier reads the stream's bytes, the frame sizes, the PCM, the index of pcm[0] and the
// handle's parameters -- nothing the encoder kept on the side.  It checks in the FORWARD direction
// (DESIGN.md §K5): from the PCM and each subframe header it recomputes what every field of the
// subframe must hold (warm-up values, residual codewords, partition parameters' positions), and
// compares those bits with the stream's.  No LPC recurrence runs: the prediction is a FIR over
// known samples, parallel over samples like K3's.
//
//   k_verify_frames  one workgroup: prefix of frame_bytes -> frame offsets, one lane per frame
//                    parses its header (sync, codes, UTF-8 number, CRC-8) and numbering/coverage
//                    is checked against the neighbouring frame -- or, with VerifyArgs.numbers, against
//                    the frame's own entry of the table; or, with VerifyArgs.block_first (variable block size,
//                    blocks of many streams), against the block the frame falls into by the sizes of the frames
//                    before it; VerifyFrame records + summary init
//   k_verify         one workgroup (256 lanes) per frame: subframes, padding, CRC-16, length
//   k_verify_final   summary[2..3] from the first failing frame; optional flag bit in totals[3]
//
// Every stream read is clamped to the frame's byte range (itself inside the stream, checked by
// k_verify_frames); every PCM index is checked against nsamples.  A corrupt stream ends in a
// status code, never in an access outside the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "flac_frame_pass.h"            // the bit reader, the header parsers, the CRCs (flac_parse.h) and the two passes
                                        // around the subframe walk: shared with K7
#include "vbs_block_lookup.h"

namespace fhip {
namespace {

constexpr int VT = 256;                // lanes per frame
constexpr int RES_CAP = 4608;           // blocks up to this keep their samples and codeword values in LDS
constexpr int FB_CAP = 12288;           // frames up to this many bytes are staged in LDS
constexpr int HDR_T = 1024;             // lanes of k_verify_frames
constexpr int ESC = 0x100;              // part_k flag: escape partition, raw width in the low bits

__device__ __forceinline__ bool fits_signed(long long v, int w)
{
    if (w <= 0) return v == 0;
    if (w >= 64) return true;
    const long long lo = -(1ll << (w - 1)), hi = (1ll << (w - 1)) - 1;
    return v >= lo && v <= hi;
}

// Compare stream bits [p, p + nb) (nb <= 64) with the low nb bits of val, MSB first.  KEY_NONE when they
// agree; else the key of the first differing bit (SAMPLES) or of the frame's end (SYNTAX: read past the end).
__device__ unsigned long long cmp_bits(const Bits &bs, long long p, int nb, uint64_t val, long long end_bits,
                                       int sub, int sample)
{
    while (nb > 0) {
        if (p >= end_bits) return mkkey(end_bits, sub, 0xFFFF, FHIP_VERIFY_SYNTAX);
        int take = nb > 32 ? 32 : nb;
        if (end_bits - p < take) take = (int)(end_bits - p);
        const uint32_t want = (uint32_t)((val >> (nb - take)) & ((take == 32) ? 0xFFFFFFFFull : ((1ull << take) - 1ull)));
        const uint32_t got = bs.rd(p, take);
        const uint32_t d = got ^ want;
        if (d) return mkkey(p + (__clz(d) - (32 - take)), sub, sample, FHIP_VERIFY_SAMPLES);
        p += take;
        nb -= take;
    }
    return KEY_NONE;
}

// q zero bits, a one, the k low bits of u
__device__ unsigned long long cmp_rice(const Bits &bs, long long p, uint32_t u, int k, long long end_bits, int sub,
                                       int sample)
{
    long long q = (long long)(u >> k);
    while (q > 0) {
        if (p >= end_bits) return mkkey(end_bits, sub, 0xFFFF, FHIP_VERIFY_SYNTAX);
        int take = q > 32 ? 32 : (int)q;
        if (end_bits - p < take) take = (int)(end_bits - p);
        const uint32_t got = bs.rd(p, take);
        if (got) return mkkey(p + (__clz(got) - (32 - take)), sub, sample, FHIP_VERIFY_SAMPLES);
        p += take;
        q -= take;
    }
    const unsigned long long r = cmp_bits(bs, p, 1, 1u, end_bits, sub, sample);
    if (r != KEY_NONE) return r;
    return k ? cmp_bits(bs, p + 1, k, u & ((1u << k) - 1u), end_bits, sub, sample) : KEY_NONE;
}

// ---- k_verify_frames -------------------------------------------------------------------------------

// BLOCKS: the block-table mode (VerifyArgs.block_first), an instance of its own -- the other is the kernel as it was;
// 2: the table's blocks differ in length (VerifyArgs.block_start), a third instance
template <int BLOCKS>
__global__ void __launch_bounds__(HDR_T) k_verify_frames(VerifyArgs a)
{
    __shared__ long long scratch[HDR_T / 64];
    __shared__ unsigned long long s_next[HDR_T];      // number + n of each frame of the chunk (VBS)
    __shared__ int s_ok[HDR_T];
    __shared__ unsigned long long s_carry_next;
    __shared__ int s_carry_ok;
    int count = a.nframes;
    if (a.dev_count) {
        const long long d = *a.dev_count;
        count = d < 0 ? 0 : (d < (long long)a.nframes ? (int)d : a.nframes);
    }
    const int t = threadIdx.x;
    const bool numbered = BLOCKS == 0 && a.numbers && !a.allow_vbs;      // a launch-wide choice: every wave takes one branch
    // block-table mode: the samples so far, and from bit BAD_SHIFT up the frames so far whose header did not parse
    // (a frame holds at most 65535 samples and a batch far fewer than 2^24 frames: the two never meet)
    constexpr int BAD_SHIFT = 40;
    long long sbase = 0;
    if (t == 0) {
        a.summary[0] = count;
        a.summary[1] = 0;
        a.key[0] = KEY_NONE;
        s_carry_next = (unsigned long long)a.first_sample;
        s_carry_ok = 1;
    }
    long long base = 0;
    for (int f0 = 0; f0 < count; f0 += HDR_T) {
        const int f = f0 + t;
        const bool live = f < count;
        VerifyFrame vf{};
        HdrOut h = frame_header<HDR_T>(a, f, live, base, scratch, vf);
        // numbering: fixed blocks carry frame numbers (frame f starts at f * block_size), a variable-block-size
        // stream carries the first sample (the frame before says where this one starts).  With a number table
        // (fixed blocks of many streams) frame f carries numbers[f] and its samples lie at f * block_size of pcm:
        // nothing of a neighbouring frame is read
        const unsigned long long snum = a.allow_vbs ? h.number : h.number * (unsigned long long)a.block_size;
        if constexpr (BLOCKS == 0) {
            s_next[t] = snum + (unsigned long long)h.n;
            s_ok[t] = h.status == FHIP_VERIFY_OK || h.status == FHIP_VERIFY_CRC8;
        }
        __syncthreads();
        // block-table mode: a frame starts where the frames before it end -- the exclusive scan of their header-parsed
        // sizes, as a sequential decoder counts -- and a frame behind one whose header did not parse cannot be placed
        long long S = 0;
        if constexpr (BLOCKS != 0) {
            const bool parsed = live && (h.status == FHIP_VERIFY_OK || h.status == FHIP_VERIFY_CRC8);
            long long stot = 0;
            S = sbase + block_excl_scan(parsed ? (long long)h.n : (live ? 1ll << BAD_SHIFT : 0ll), scratch, HDR_T / 64, &stot);
            sbase += stot;
        }
        if (live && (h.status == FHIP_VERIFY_OK || h.status == FHIP_VERIFY_CRC8)) {
            long long rel;
            bool num_ok, cover_ok;
            if constexpr (BLOCKS != 0) {
                // the frame lies in block S / block_size at offset S % block_size; the table says what the first
                // sample of that block is called in its own stream.  Only the sample count so far crosses frames.
                const bool placeable = (S >> BAD_SHIFT) == 0;
                S &= (1ll << BAD_SHIFT) - 1;
                long long blk, bstart, blen = a.block_size;
                if constexpr (BLOCKS == 2) {
                    // a length per block: the block is found in the prefix sums of the lengths (vbs_block_lookup.h)
                    blk = fhip_block_lookup(a.block_start, a.nblocks, S);
                    const long long bq = blk < (long long)a.nblocks ? blk : 0;      // (an index inside the table either way)
                    bstart = a.block_start[bq];
                    blen = a.block_start[bq + 1] - bstart;
                } else {
                    blk = S / a.block_size;
                    bstart = blk * a.block_size;
                }
                const int off = (int)(S - bstart);
                const bool placed = placeable && blk < (long long)a.nblocks;
                rel = S;
                num_ok = !placed || h.number == (unsigned long long)(uint32_t)(a.block_first[blk] + (uint32_t)off);
                cover_ok = placed && off + h.n <= blen && (f != count - 1 || S + h.n == a.nsamples);
            } else if (numbered) {
                // every frame is a whole block of its own stream: the table says which, the batch says where
                // (ragged: the tables say where and how long; frame_src counts interleaved values)
                rel = a.frame_src ? a.frame_src[f] / a.channels : (long long)f * a.block_size;
                num_ok = h.number == (unsigned long long)a.numbers[f];
                cover_ok = h.n == (a.frame_n ? a.frame_n[f] : a.block_size);
            } else if (!a.allow_vbs) {
                rel = (long long)f * a.block_size;
                num_ok = snum == (unsigned long long)(a.first_sample + rel);
                cover_ok = (f == count - 1) ? (rel + h.n == a.nsamples) : (h.n == a.block_size);
            } else {
                // (a frame whose own header is broken has already failed: its successor is not blamed for it)
                const unsigned long long prev_next = t ? s_next[t - 1] : s_carry_next;
                const int prev_ok = t ? s_ok[t - 1] : s_carry_ok;
                const unsigned long long want = f == 0 ? (unsigned long long)a.first_sample : (prev_ok ? prev_next : snum);
                rel = (long long)(snum - (unsigned long long)a.first_sample);
                num_ok = snum == want;
                cover_ok = (f == count - 1) ? (rel + h.n == a.nsamples) : true;
            }
            cover_ok = cover_ok && rel >= 0 && rel <= a.nsamples && h.n <= a.nsamples - rel;
            if (!num_ok) { h.status = FHIP_VERIFY_NUMBER; h.bit = 32; }
            else if (!cover_ok) { h.status = FHIP_VERIFY_NUMBER; h.bit = 16; }
            vf.rel_start = rel;
        }
        if (live) {
            frame_fill(vf, h);
            a.ws[f] = vf;
        }
        __syncthreads();
        if (t == HDR_T - 1) { s_carry_next = s_next[t]; s_carry_ok = s_ok[t]; }
        __syncthreads();
    }
}

// ---- k_verify --------------------------------------------------------------------------------------

__device__ __forceinline__ long long pcm_at(const VerifyArgs &a, long long g, int c)
{
    if (g < 0 || g >= a.nsamples) return 0;          // (pass 1 keeps every frame inside [0, nsamples))
    // the caller's PCM at the handle's width (fhip_set_pcm_format)
    if (a.pcm_format == FHIP_PCM_S16) return (long long)reinterpret_cast<const int16_t *>(a.pcm)[g * a.channels + c];
    return (long long)a.pcm[g * a.channels + c];
}

// the subframe's value before wasted-bit removal: the frame's channel transform of the input.  Samples are
// restored wrapped to int32 (as the oracle decoder and libFLAC's 32-bit output do), so the side channel of a
// 32-bit stream is L - R wrapped to int32 -- a no-op below 32 bits
__device__ __forceinline__ long long wrap32(long long v) { return (long long)(int32_t)(uint32_t)(uint64_t)v; }
__device__ __forceinline__ long long chan_at(const VerifyArgs &a, long long g, int ch_code, int c)
{
    if (ch_code < 8) return pcm_at(a, g, c);
    const long long l = pcm_at(a, g, 0), r = pcm_at(a, g, 1);
    if (ch_code == FHIP_CH_LEFT_SIDE) return c == 0 ? l : wrap32(l - r);
    if (ch_code == FHIP_CH_RIGHT_SIDE) return c == 0 ? wrap32(l - r) : r;
    return c == 0 ? ((l + r) >> 1) : wrap32(l - r);   // mid / side
}

// A raw value field of w bits (warm-up, VERBATIM, CONSTANT).  A 33-bit field (the side channel of a 32-bit
// stream) is read wrapped to int32: only its low 32 bits carry the value.
__device__ unsigned long long cmp_raw(const Bits &bs, long long p, int w, long long v, long long end, int sub,
                                      int sample)
{
    if (!fits_signed(v, w)) return mkkey(p, sub, sample, FHIP_VERIFY_SAMPLES);
    if (w > 32) { p += w - 32; w = 32; }
    return cmp_bits(bs, p, w, (uint64_t)v, end, sub, sample);
}

struct Ctx {
    const VerifyArgs *a;
    long long g0;          // absolute PCM index (relative to pcm[0]) of the frame's first sample
    int ch_code, c, n;
    bool resident;
    const int32_t *y;      // LDS values after wasted-bit removal (resident)
    const uint32_t *zz;    // LDS zig-zag residuals (resident)
    const SubHdr *sh;
};

__device__ __forceinline__ long long y_at(const Ctx &x, int i)
{
    if (x.resident) return x.y[i];
    return chan_at(*x.a, x.g0 + i, x.ch_code, x.c) >> x.sh->wasted;
}

// residual e_i of a FIXED / LPC subframe at sample i >= order: the int32 e with (int32)(e + prediction) = sample
__device__ long long resid_at(const Ctx &x, int i, bool *ok)
{
    const SubHdr &s = *x.sh;
    long long pred = 0;
    if (s.type == FHIP_SUB_FIXED) {
        switch (s.order) {
        case 1: pred = y_at(x, i - 1); break;
        case 2: pred = 2 * y_at(x, i - 1) - y_at(x, i - 2); break;
        case 3: pred = 3 * y_at(x, i - 1) - 3 * y_at(x, i - 2) + y_at(x, i - 3); break;
        case 4: pred = 4 * y_at(x, i - 1) - 6 * y_at(x, i - 2) + 4 * y_at(x, i - 3) - y_at(x, i - 4); break;
        default: break;
        }
    } else {
        long long acc = 0;
        for (int j = 0; j < s.order; j++) acc += (long long)s.coef[j] * y_at(x, i - 1 - j);
        pred = acc >> s.shift;
    }
    *ok = true;
    return wrap32(y_at(x, i) - pred);
}

__device__ __forceinline__ uint32_t zigzag(long long e)
{
    const int32_t v = (int32_t)e;
    return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31);
}

__device__ __forceinline__ uint32_t zz_at(const Ctx &x, int i)
{
    if (x.resident) return x.zz[i];
    bool ok;
    return zigzag(resid_at(x, i, &ok));
}

__global__ void __launch_bounds__(VT) k_verify(VerifyArgs a)
{
    __shared__ int32_t y_lds[RES_CAP];
    __shared__ uint32_t zz_lds[RES_CAP];
    __shared__ uint8_t fb_lds[FB_CAP];
    __shared__ long long part_base[FHIP_MAX_PARTS];
    __shared__ int part_k[FHIP_MAX_PARTS];
    __shared__ long long scratch[VT / 64];
    __shared__ SubHdr s_sh;
    __shared__ unsigned long long s_key;
    __shared__ int s_bad, s_walked;
    __shared__ long long s_pos, s_wP, s_wQ;
    __shared__ int s_stop;
    __shared__ uint32_t s_crc;

    const int f = blockIdx.x, t = threadIdx.x;
    if (a.dev_count && (long long)f >= *a.dev_count) return;
    const VerifyFrame vf = a.ws[f];
    unsigned long long key = KEY_NONE;
    if (vf.status != FHIP_VERIFY_OK) {
        key = mkkey(vf.bit, 15, 0xFFFF, vf.status);
    } else {
        const Bits bs = frame_stage<VT>(fb_lds, a.stream + vf.off, vf.bytes);
        const long long end = (long long)vf.bytes * 8;
        const int n = vf.n;
        const int nch = a.channels;
        if (t == 0) { s_key = KEY_NONE; s_pos = vf.hdr_bits; }
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            __syncthreads();                   // everybody is done with the previous subframe's shared state
            const int sub_bps = subframe_bps(a.bps, vf.ch_code, c);
            if (t == 0) {
                const unsigned long long k = parse_subframe(bs, s_pos, end, sub_bps, n, &s_sh, c);
                if (k != KEY_NONE) s_key = k;
                s_bad = n;
            }
            __syncthreads();
            if (s_key != KEY_NONE) break;
            const SubHdr &sh = s_sh;
            const bool resident = n <= RES_CAP;
            Ctx x{&a, vf.rel_start, vf.ch_code, c, n, resident, y_lds, zz_lds, &sh};
            // the values the subframe must carry; the first sample with set wasted bits has no encoding
            const long long wmask = (1ll << sh.wasted) - 1;
            for (int i = t; i < n; i += VT) {
                const long long v = chan_at(a, vf.rel_start + i, vf.ch_code, c);
                if (v & wmask) atomicMin(&s_bad, i);
                if (resident) y_lds[i] = (int32_t)(v >> sh.wasted);
            }
            __syncthreads();
            const int bad = s_bad;
            const int w = sh.w;
            unsigned long long mine = KEY_NONE;
            long long sub_end = 0;
            if (sh.type == FHIP_SUB_CONSTANT) {
                if (t == 0) {
                    const long long v0 = y_at(x, 0);
                    mine = bad == 0 ? mkkey(sh.pos, c, 0, FHIP_VERIFY_SAMPLES) : cmp_raw(bs, sh.pos, w, v0, end, c, 0);
                }
                if (mine == KEY_NONE) {
                    const long long v0 = y_at(x, 0);
                    for (int i = t; i < n; i += VT)
                        if (i == bad || y_at(x, i) != v0) { mine = mkkey(sh.pos, c, i, FHIP_VERIFY_SAMPLES); break; }
                }
                sub_end = sh.pos + w;
            } else {
                const int nraw = sh.type == FHIP_SUB_VERBATIM ? n : sh.order;
                for (int i = t; i < nraw && mine == KEY_NONE; i += VT) {
                    const long long v = y_at(x, i), p = sh.pos + (long long)i * w;
                    mine = i == bad ? mkkey(p, c, i, FHIP_VERIFY_SAMPLES) : cmp_raw(bs, p, w, v, end, c, i);
                }
                sub_end = sh.pos + (long long)nraw * w;
            }
            if (sh.type == FHIP_SUB_FIXED || sh.type == FHIP_SUB_LPC) {
                const int order = sh.order;
                if (resident) {
                    for (int i = order + t; i < n; i += VT) {
                        bool ok;
                        zz_lds[i] = zigzag(resid_at(x, i, &ok));
                    }
                }
                __syncthreads();
                const int npart = 1 << sh.porder, psz = n >> sh.porder;
                const int pbits = sh.method ? 5 : 4, esc = sh.method ? 31 : 15;
                // partitions in groups of FHIP_MAX_PARTS (FLAC allows partition order 15): the walk over a group's
                // parameters and lengths (one wave, a step per partition), then every lane checks its codewords
                if (t == 0) { s_wP = sh.res + 6; s_wQ = 0; s_stop = 0; }
                __syncthreads();
                for (int g0 = 0; g0 < npart; g0 += FHIP_MAX_PARTS) {
                    const int g1 = min(npart, g0 + FHIP_MAX_PARTS);
                    const long long Qbase = s_wQ;           // codeword bits of the groups before
                    const long long P0 = s_wP;
                    __syncthreads();
                    if (t < 64) {
                        long long P = P0, Q = Qbase;
                        int walked = g0;
                        unsigned long long wkey = KEY_NONE;
                        for (int j = g0; j < g1; j++) {
                            if (P + pbits > end) { wkey = mkkey(end, c, 0xFFFF, FHIP_VERIFY_SYNTAX); break; }
                            int k = (int)bs.rd(P, pbits);
                            P += pbits;
                            const int s0 = j ? j * psz : order, s1 = (j + 1) * psz;
                            long long len;
                            if (k == esc) {
                                if (P + 5 > end) { wkey = mkkey(end, c, 0xFFFF, FHIP_VERIFY_SYNTAX); break; }
                                const int raw = (int)bs.rd(P, 5);
                                P += 5;
                                k = ESC | raw;
                                len = (long long)(s1 - s0) * raw;
                            } else {
                                long long sum = 0;
                                for (int i = s0 + t; i < s1; i += 64) sum += zz_at(x, i) >> k;
                                for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
                                len = sum + (long long)(s1 - s0) * (1 + k);
                            }
                            if (t == 0) { part_base[j - g0] = P - Q; part_k[j - g0] = k; }
                            P += len;
                            Q += len;
                            walked = j + 1;
                        }
                        if (t == 0) {
                            s_walked = walked;
                            s_wP = P;
                            s_wQ = Q;
                            if (wkey != KEY_NONE) { atomicMin(&s_key, wkey); s_stop = 1; }
                        }
                    }
                    __syncthreads();
                    const int walked = s_walked;
                    const int lo = g0 ? g0 * psz : order;
                    const int lim = walked * psz;                   // samples whose partitions were read
                    const int nres = lim > lo ? lim - lo : 0;
                    const int seg = (nres + VT - 1) / VT;
                    const int i0 = lo + t * seg, i1 = min(i0 + seg, lim);
                    long long lsum = 0;
                    for (int i = i0; i < i1; i++) {
                        const int k = part_k[i / psz - g0];
                        lsum += (k & ESC) ? (k & 31) : (long long)(zz_at(x, i) >> k) + 1 + k;
                    }
                    long long tot;
                    long long Qi = Qbase + block_excl_scan(lsum, scratch, VT / 64, &tot);
                    for (int i = i0; i < i1 && mine == KEY_NONE; i++) {
                        const int j = i / psz - g0, k = part_k[j];
                        const long long p = part_base[j] + Qi;
                        bool ok;
                        const long long e = resid_at(x, i, &ok);
                        if (i == bad || !ok) { mine = mkkey(p, c, i, FHIP_VERIFY_SAMPLES); break; }
                        if (k & ESC) {
                            const int raw = k & 31;
                            mine = fits_signed(e, raw) ? cmp_bits(bs, p, raw, (uint64_t)e, end, c, i)
                                                       : mkkey(p, c, i, FHIP_VERIFY_SAMPLES);
                            Qi += raw;
                        } else {
                            const uint32_t u = zigzag(e);
                            mine = cmp_rice(bs, p, u, k, end, c, i);
                            Qi += (long long)(u >> k) + 1 + k;
                        }
                    }
                    if (mine != KEY_NONE) atomicMin(&s_key, mine);
                    mine = KEY_NONE;
                    __syncthreads();
                    const bool stop = s_stop || s_key != KEY_NONE;
                    __syncthreads();
                    if (stop) break;
                }
                if (t == 0) s_pos = s_wP;
            } else if (t == 0) {
                s_pos = sub_end;
            }
            if (mine != KEY_NONE) atomicMin(&s_key, mine);
            __syncthreads();
            if (s_key != KEY_NONE) break;
        }
        key = frame_tail<VT>(bs, vf.bytes, s_key, s_pos, s_crc);
    }
    if (t == 0) frame_record<true>(a.recs, a.summary, a.key, f, key);
}

__global__ void k_verify_final(VerifyArgs a)
{
    if (frame_summary_end(a.key[0], a.summary) && a.totals) a.totals[3] |= 4;
}

}  // namespace

hipError_t launch_verify(hipStream_t st, const VerifyArgs &a)
{
    if (a.block_first && a.block_start && a.allow_vbs && a.nblocks > 0) {
        note_launch("k_verify_frames<blocks ragged>");
        hipLaunchKernelGGL(k_verify_frames<2>, dim3(1), dim3(HDR_T), 0, st, a);
    } else if (a.block_first && a.allow_vbs) {
        note_launch("k_verify_frames<blocks>");
        hipLaunchKernelGGL(k_verify_frames<1>, dim3(1), dim3(HDR_T), 0, st, a);
    } else {
        note_launch("k_verify_frames");
        hipLaunchKernelGGL(k_verify_frames<0>, dim3(1), dim3(HDR_T), 0, st, a);
    }
    if (a.nframes > 0) {
        note_launch("k_verify");
        hipLaunchKernelGGL(k_verify, dim3(a.nframes), dim3(VT), 0, st, a);
    }
    note_launch("k_verify_final");
    hipLaunchKernelGGL(k_verify_final, dim3(1), dim3(1), 0, st, a);
    return hipGetLastError();
}

}  // namespace fhip
