// flac_frame_pass.h -- what K5 (k5_verify.hip) and K7 (k7_frame.h) do alike around a frame's subframes, on top of
// flac_parse.h: the header pass's prologue (where the frame lies, whether it fits the stream, its parsed header), and of
// the frame pass the staging in LDS, the side channel's width, the tail behind the last subframe (padding, CRC-16,
// length), the record and summary write-out and the end kernels' body.  The subframe walks stay with their kernels: K5
// checks forward over known samples, K7 runs the recurrence.  T is the lane count of the calling workgroup; what only a
// workgroup of several waves needs is under if constexpr.  Everything is internal to the including file.
#pragma once

#include "flac_parse.h"

namespace fhip {
namespace {

// ---- the header pass: one lane per frame of a chunk of T --------------------------------------------

// Frame f's offset (base: the bytes of the chunks before, moved on by this chunk's) and its header.  a: the stream, the
// frame sizes and what parse_header holds the codes against.  A frame without bytes, or one that ends behind the stream,
// fails with LENGTH and is never read.  Every lane of the workgroup calls (the scan has barriers).
template <int T>
__device__ __forceinline__ HdrOut frame_header(const VerifyArgs &a, int f, bool live, long long &base, long long *scratch,
                                               VerifyFrame &vf)
{
    const long long fb = live ? (long long)a.frame_bytes[f] : 0;
    long long tot = 0;
    const long long off = base + block_excl_scan(fb > 0 ? fb : 0, scratch, T / 64, &tot);
    base += tot;
    vf.off = off;
    vf.bytes = (int)fb;
    HdrOut h{FHIP_VERIFY_OK, 0, 0, 0, 0, 0};
    if (live) {
        if (fb <= 0 || off + fb > a.stream_bytes) {
            h.status = FHIP_VERIFY_LENGTH;
            h.bit = fb <= 0 ? 0 : (a.stream_bytes - off) * 8;
            if (h.bit < 0) h.bit = 0;
        } else {
            h = parse_header(a, Bits{a.stream + off, fb});
        }
    }
    return h;
}

// what the frame pass needs of the header (rel_start is the caller's)
__device__ __forceinline__ void frame_fill(VerifyFrame &vf, const HdrOut &h)
{
    vf.n = h.n;
    vf.hdr_bits = h.hdr_bits;
    vf.ch_code = h.ch_code;
    vf.status = h.status;
    vf.bit = h.bit;
}

// ---- the frame pass: T lanes per frame ---------------------------------------------------------------

// the frame's bytes (the header pass put them inside the stream): staged in LDS when they fit
template <int T, int CAP>
__device__ __forceinline__ Bits frame_stage(uint8_t (&fb_lds)[CAP], const uint8_t *src, int bytes)
{
    const bool staged = bytes <= CAP;
    if (staged)
        for (int i = threadIdx.x; i < bytes; i += T) fb_lds[i] = src[i];
    return Bits{staged ? fb_lds : src, bytes};
}

// subframe c's sample width: the side channel carries a bit more
__device__ __forceinline__ int subframe_bps(int bps, int ch_code, int c)
{
    const bool side = (ch_code == FHIP_CH_LEFT_SIDE && c == 1) || (ch_code == FHIP_CH_RIGHT_SIDE && c == 0) ||
                      (ch_code == FHIP_CH_MID_SIDE && c == 1);
    return bps + (side ? 1 : 0);
}

// Behind the last subframe: padding to the byte, CRC-16, the end.  s_key, s_pos and s_crc are the workgroup's (LDS): the
// key of the subframes' first failure or KEY_NONE, and the bit the last subframe ended at; a barrier lies behind their
// last write.  Returns the frame's key, to every lane.
template <int T>
__device__ __forceinline__ unsigned long long frame_tail(const Bits &bs, int bytes, unsigned long long &s_key,
                                                         const long long &s_pos, uint32_t &s_crc)
{
    const int t = threadIdx.x;
    const long long end = (long long)bytes * 8;
    const bool clean = s_key == KEY_NONE;
    __syncthreads();
    if (clean) {
        const long long p = s_pos;
        const long long body = (p + 7) >> 3;                      // bytes the CRC-16 covers
        if (t == 0) {
            unsigned long long k = KEY_NONE;
            if (p > end) k = mkkey(end, 15, 0xFFFF, FHIP_VERIFY_SYNTAX);
            else if (body * 8 > p && bs.rd(p, (int)(body * 8 - p)) != 0) {
                const int nb = (int)(body * 8 - p);
                const uint32_t v = bs.rd(p, nb);
                k = mkkey(p + (__clz(v) - (32 - nb)), 15, 0xFFFF, FHIP_VERIFY_PADDING);
            } else if (body + 2 > bytes) {
                k = mkkey(end, 15, 0xFFFF, FHIP_VERIFY_LENGTH);
            }
            s_key = k;
            s_crc = 0;
        }
        __syncthreads();
        const bool framed = s_key == KEY_NONE;
        __syncthreads();
        if (framed) {
            // CRC-16 of [0, body): a chunk per lane, moved to the end of the body in GF(2) and xor-ed
            const long long L = (body + T - 1) / T;
            const long long b0 = (long long)t * L, b1 = min(b0 + L, body);
            uint32_t crc = 0;
            for (long long i = b0; i < b1; i++) crc = crc16_byte(crc, bs.byte(i));
            if (b0 < b1 && crc) crc = gf16_mul(crc, gf16_xpow8(body - b1));
            for (int d = 32; d > 0; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
            if constexpr (T > 64) {
                if ((t & 63) == 0 && crc) atomicXor(&s_crc, crc);
                __syncthreads();
            }
            if (t == 0) {
                const uint32_t got = bs.rd(body * 8, 16);
                if (got != (T > 64 ? s_crc : crc)) s_key = mkkey(body * 8, 15, 0xFFFF, FHIP_VERIFY_CRC16);
                else if (body + 2 != bytes) s_key = mkkey((body + 2) * 8, 15, 0xFFFF, FHIP_VERIFY_LENGTH);
            }
        }
    }
    __syncthreads();
    return s_key;
}

// one lane: frame f's record and its share of the summary.  SAMPLE: the key names a sample (K5's SAMPLES status).
template <bool SAMPLE>
__device__ __forceinline__ void frame_record(fhip_verify_rec *recs, long long *summary, unsigned long long *first, int f,
                                             unsigned long long key)
{
    const int status = key == KEY_NONE ? FHIP_VERIFY_OK : (int)(key & 15);
    if (recs) {
        fhip_verify_rec r;
        r.status = status;
        r.bit = status == FHIP_VERIFY_OK ? -1 : (int32_t)min((long long)(key >> 24), 0x7FFFFFFFll);
        const int sub = (int)((key >> 20) & 15), smp = (int)((key >> 4) & 0xFFFF);
        r.subframe = (status == FHIP_VERIFY_OK || sub == 15) ? -1 : sub;
        r.sample = (SAMPLE && status == FHIP_VERIFY_SAMPLES && smp != 0xFFFF) ? smp : -1;
        recs[f] = r;
    }
    if (status != FHIP_VERIFY_OK) {
        atomicAdd((unsigned long long *)&summary[1], 1ull);
        atomicMin(first, ((unsigned long long)f << 8) | (unsigned long long)status);
    }
}

// the end kernels: summary[2..3] from the first failing frame; whether there is one
__device__ __forceinline__ bool frame_summary_end(unsigned long long k, long long *summary)
{
    summary[2] = k == KEY_NONE ? -1 : (long long)(k >> 8);
    summary[3] = k == KEY_NONE ? 0 : (long long)(k & 0xFF);
    return k != KEY_NONE;
}

}  // namespace
}  // namespace fhip
