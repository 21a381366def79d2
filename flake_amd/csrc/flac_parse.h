// flac_parse.h -- reading a FLAC frame on the device.  For K5 (k5_verify.hip, the verifier) and K7 (k7_decode.hip, the
// decoder): a clamped MSB-first bit reader, the discrepancy key, the frame-header parser that says where and why a
// header fails (its tables and its CRC-8 step are flac_header.h's) and the subframe-header parser.  For those two and
// K8 (k8_index.hip, frame discovery): CRC-16 a byte at a time and as GF(2) products (a chunk per lane, moved to its
// place) and the workgroup's exclusive scan.  Everything is internal to the including file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flac_header.h"
#include "kernels.h"

namespace fhip {
namespace {

constexpr unsigned long long KEY_NONE = ~0ull;

// key: bit position, then subframe, then sample, then status -- the minimum is the first discrepancy
__device__ __forceinline__ unsigned long long mkkey(long long pos, int sub, int sample, int status)
{
    if (pos < 0) pos = 0;
    if (pos > 0xFFFFFFFFFFll) pos = 0xFFFFFFFFFFll;
    return ((unsigned long long)pos << 24) | ((unsigned long long)(sub & 15) << 20) |
           ((unsigned long long)(sample & 0xFFFF) << 4) | (unsigned long long)(status & 15);
}

// MSB-first bit reader over [0, nbytes) of src; bytes past the end read as zero
struct Bits {
    const uint8_t *src;
    long long nbytes;
    __device__ __forceinline__ uint32_t byte(long long i) const { return (i >= 0 && i < nbytes) ? src[i] : 0u; }
    // nb in 0..32
    __device__ __forceinline__ uint32_t rd(long long p, int nb) const
    {
        if (nb <= 0) return 0u;
        const long long b = p >> 3;
        uint64_t w = 0;
        for (int t = 0; t < 5; t++) w = (w << 8) | byte(b + t);
        const int sh = 40 - (int)(p & 7) - nb;
        return (uint32_t)((w >> sh) & (nb == 32 ? 0xFFFFFFFFull : ((1ull << nb) - 1ull)));
    }
};

__device__ __forceinline__ uint32_t crc16_byte(uint32_t c, uint32_t b)
{
    c ^= b << 8;
    for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
    return c & 0xFFFFu;
}

// a * b mod the CRC-16 polynomial x^16 + x^15 + x^2 + 1 (GF(2)); a, b < 2^16.  Also for static_asserts.
__host__ __device__ __forceinline__ constexpr uint32_t gf16_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 15; i >= 0; i--) {
        r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) : (r << 1);
        if ((b >> i) & 1u) r ^= a;
    }
    return r & 0xFFFFu;
}

// x^(8 m) mod the polynomial: the factor that moves a chunk's CRC past m further bytes
__device__ uint32_t gf16_xpow8(long long m)
{
    uint32_t r = 1u, b = 0x100u;        // x^8
    while (m > 0) {
        if (m & 1) r = gf16_mul(r, b);
        b = gf16_mul(b, b);
        m >>= 1;
    }
    return r;
}

// ---- the frame header ------------------------------------------------------------------------------

struct HdrOut { int status; long long bit; int n; int hdr_bits; int ch_code; unsigned long long number; };

// Not flac_header_ok's yes or no but where the first check fails, and which.  a: channels, bps, sample_rate and
// block_size are what the header codes are held against (block_size is the largest block, and always a limit);
// allow_vbs is the blocking-strategy bit the frame must carry.
__device__ HdrOut parse_header(const VerifyArgs &a, const Bits &bs)
{
    HdrOut h{FHIP_VERIFY_OK, 0, 0, 0, 0, 0};
    const long long end = bs.nbytes * 8;
#define VFAIL(pos, st) do { h.status = (st); h.bit = (pos); return h; } while (0)
#define NEED(pos, nb) do { if ((pos) + (nb) > end) VFAIL(end, FHIP_VERIFY_SYNTAX); } while (0)
    NEED(0, 32);
    const uint32_t w = bs.rd(0, 32);
    const uint32_t sync = w >> 18;
    if (sync != 0x3FFEu) VFAIL(__clz((sync ^ 0x3FFEu) << 18), FHIP_VERIFY_HEADER);
    if ((w >> 17) & 1u) VFAIL(14, FHIP_VERIFY_HEADER);
    if ((int)((w >> 16) & 1u) != (a.allow_vbs ? 1 : 0)) VFAIL(15, FHIP_VERIFY_HEADER);
    const int bs_code = (int)((w >> 12) & 15u), sr_code = (int)((w >> 8) & 15u);
    const int ch_code = (int)((w >> 4) & 15u), bps_code = (int)((w >> 1) & 7u);
    if (bs_code == 0) VFAIL(16, FHIP_VERIFY_HEADER);
    int n = flac_block_size_of_code(bs_code);
    if (n && n > a.block_size) VFAIL(16, FHIP_VERIFY_NUMBER);
    if (sr_code == 15 || (sr_code < 12 && !flac_rate_code_ok(sr_code, a.sample_rate))) VFAIL(20, FHIP_VERIFY_HEADER);
    if (ch_code > 10 || (ch_code < 8 && ch_code + 1 != a.channels) || (ch_code >= 8 && a.channels != 2))
        VFAIL(24, FHIP_VERIFY_HEADER);
    if (bps_code != 0 && bps_code != flac_bps_code(a.bps)) VFAIL(28, FHIP_VERIFY_HEADER);
    if (w & 1u) VFAIL(31, FHIP_VERIFY_HEADER);
    // UTF-8 style number: 1 .. 7 bytes, up to 36 bits
    long long p = 32;
    NEED(p, 8);
    const uint32_t b0 = bs.rd(p, 8);
    int extra = 0;
    unsigned long long num = 0;
    if (b0 < 0x80u) {
        num = b0;
    } else {
        int ones = 0;
        while (ones < 8 && ((b0 << ones) & 0x80u)) ones++;
        if (ones < 2 || ones > 7) VFAIL(p, FHIP_VERIFY_HEADER);
        extra = ones - 1;
        num = (ones == 7) ? 0 : (b0 & (0x7Fu >> ones));
    }
    p += 8;
    for (int i = 0; i < extra; i++) {
        NEED(p, 8);
        const uint32_t c = bs.rd(p, 8);
        if ((c & 0xC0u) != 0x80u) VFAIL(p, FHIP_VERIFY_HEADER);
        num = (num << 6) | (c & 0x3Fu);
        p += 8;
    }
    if (bs_code == 6 || bs_code == 7) {
        const int nb = bs_code == 6 ? 8 : 16;
        NEED(p, nb);
        n = (int)bs.rd(p, nb) + 1;
        if (n > a.block_size || n > FHIP_MAX_BLOCK) VFAIL(p, FHIP_VERIFY_NUMBER);
        p += nb;
    }
    if (sr_code >= 12) {
        const int nb = sr_code == 12 ? 8 : 16;
        NEED(p, nb);
        const long long v = bs.rd(p, nb);
        const long long rate = sr_code == 12 ? v * 1000 : (sr_code == 13 ? v : v * 10);
        if (rate != a.sample_rate) VFAIL(p, FHIP_VERIFY_HEADER);
        p += nb;
    }
    NEED(p, 8);
    uint32_t c8 = 0;
    for (long long i = 0; i < (p >> 3); i++) c8 = flac_crc8_step(c8, bs.byte(i));
    if (bs.rd(p, 8) != c8) VFAIL(p, FHIP_VERIFY_CRC8);
    h.n = n;
    h.hdr_bits = (int)(p + 8);
    h.ch_code = ch_code;
    h.number = num;
    return h;
#undef NEED
#undef VFAIL
}

__device__ long long block_excl_scan(long long v, long long *scratch, int nwaves, long long *total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) scratch[wid] = incl;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int q = 0; q < nwaves; q++) {
        const long long s = scratch[q];
        if (q < wid) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// ---- the subframe header ---------------------------------------------------------------------------

struct SubHdr {
    int type;          // FHIP_SUB_*
    int order, wasted, w, shift, method, porder;
    long long pos;     // CONSTANT: the value; VERBATIM / FIXED / LPC: the first warm-up (or verbatim) value
    long long res;     // FIXED / LPC: the residual section (method bits)
    int coef[FHIP_MAX_ORDER];
};

// one lane: the subframe header at pos.  Returns KEY_NONE or the key of a syntax error.
__device__ unsigned long long parse_subframe(const Bits &bs, long long pos, long long end, int sub_bps, int n,
                                             SubHdr *s, int sub)
{
#define SFAIL(p) return mkkey((p), sub, 0xFFFF, FHIP_VERIFY_SYNTAX)
#define SNEED(p, nb) do { if ((p) + (nb) > end) SFAIL(end); } while (0)
    long long p = pos;
    SNEED(p, 8);
    const uint32_t h = bs.rd(p, 8);
    if (h & 0x80u) SFAIL(p);
    const int t = (int)((h >> 1) & 63u);
    p += 8;
    int wasted = 0;
    if (h & 1u) {
        // unary count of wasted bits - 1
        int k = 0;
        for (;;) {
            SNEED(p, 1);
            const uint32_t bit = bs.rd(p, 1);
            p++;
            if (bit) break;
            if (++k >= sub_bps) SFAIL(p - 1);
        }
        wasted = k + 1;
        if (wasted >= sub_bps) SFAIL(p - 1);
    }
    s->wasted = wasted;
    s->w = sub_bps - wasted;
    s->order = 0; s->shift = 0; s->method = 0; s->porder = 0; s->res = 0;
    if (t == 0) {
        s->type = FHIP_SUB_CONSTANT;
    } else if (t == 1) {
        s->type = FHIP_SUB_VERBATIM;
    } else if (t >= 8 && t <= 12) {
        s->type = FHIP_SUB_FIXED;
        s->order = t - 8;
    } else if (t >= 32) {
        s->type = FHIP_SUB_LPC;
        s->order = t - 31;
    } else {
        SFAIL(pos + 1);
    }
    s->pos = p;
    if (s->type == FHIP_SUB_CONSTANT || s->type == FHIP_SUB_VERBATIM) return KEY_NONE;
    if (s->order > n) SFAIL(pos + 1);
    p += (long long)s->order * s->w;
    if (s->type == FHIP_SUB_LPC) {
        SNEED(p, 9);
        const int prec = (int)bs.rd(p, 4) + 1;
        if (prec == 16) SFAIL(p);
        p += 4;
        const uint32_t sh = bs.rd(p, 5);
        if (sh & 0x10u) SFAIL(p);                          // negative shift
        s->shift = (int)sh;
        p += 5;
        SNEED(p, (long long)s->order * prec);
        for (int j = 0; j < s->order; j++) {
            uint32_t v = bs.rd(p, prec);
            if (prec < 32 && (v & (1u << (prec - 1)))) v |= ~((1u << prec) - 1u);
            s->coef[j] = (int32_t)v;
            p += prec;
        }
    }
    SNEED(p, 6);
    s->res = p;
    const uint32_t m = bs.rd(p, 6);
    s->method = (int)(m >> 4);
    s->porder = (int)(m & 15u);
    if (s->method > 1) SFAIL(p);
    if ((n & ((1 << s->porder) - 1)) || (n >> s->porder) < s->order) SFAIL(p + 2);
    return KEY_NONE;
#undef SNEED
#undef SFAIL
}

}  // namespace
}  // namespace fhip
