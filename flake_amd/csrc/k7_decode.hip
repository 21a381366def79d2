// k7_decode.hip -- K7: FLAC frames back to PCM.
//
// The inverse of the encode path, by the FLAC format alone: a batch of frames whose byte sizes are known is
// parsed, its residuals are read, the prediction recurrence runs and the channel transform is undone.  Laid out
// like K5 (k5_verify.hip), with which it shares the bit reader and the header parsers (flac_parse.h):
//
//   k_decode_frames  one workgroup: prefix of frame_bytes -> frame offsets, one lane per frame parses its
//                    header (sync, codes, UTF-8 number, CRC-8); the scan of the parsed block sizes says where
//                    each frame's samples go; numbering is held against the neighbouring frame (and the
//                    first frame against first_number), a frame that would not fit pcm_cap is refused;
//                    VerifyFrame records + summary init + the sample count
//   k_decode         one wave per frame.  Inside a frame the parse is sequential (a Rice code's length is known
//                    once its unary part is read, subframe c starts where c - 1 ends), so one lane walks the
//                    bits; it restores each sample as it reads its residual, the history in an LDS ring, and
//                    the wave stores 64 restored samples at a time into the frame's rows of the handle's
//                    sample workspace.  Raw fields (CONSTANT, VERBATIM, warm-up) are read by all lanes.
//                    Then padding, CRC-16 (a chunk per lane, moved in GF(2)) and the length; a frame that
//                    passed is written out by all lanes: wasted-bit shift, channel recombination, interleave.
//   k_decode_final   summary[2..3] from the first failing frame
//
// Every stream read is clamped to the frame's byte range (itself inside the stream, checked by
// k_decode_frames); a partition never yields more residuals than the block has left (the walk is driven by
// the sample index, not by the stream); every PCM write is inside [0, pcm_cap) and inside the frame's own
// sample range; every row write is inside the frame's own rows.  A corrupt stream ends in a status code.
//
// The window mode (FHIP_K7_WINDOWS): k7_decode_windows.hip defines the macro and includes this file, which then makes
// k_decode_frames_windows and k_decode_windows of the same text instead of the kernels above, and launch_decode_windows
// instead of launch_decode.  Segment s delivers only samples [seg_skip[s], seg_skip[s] + seg_take[s]) of its own, counted
// over the sizes of its good headers.  Every frame is still parsed, restored and checked in full; what changes is where a
// frame's samples go and which of them: the header pass leaves a DecodeClip per frame, and the write-out of the frame
// pass runs over the clip alone.  Every difference is under #if, so that without the macro this file is, token for
// token, what it was: the register and LDS figures of its kernels are pinned by tests.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "flac_parse.h"

#ifndef FHIP_K7_WINDOWS
#define FHIP_K7_WINDOWS 0
#endif

namespace fhip {
namespace {

constexpr int DT = 64;                  // lanes per frame: one wave
constexpr int DFB_CAP = 16384;          // frames up to this many bytes are staged in LDS
constexpr int DHDR_T = 1024;            // lanes of k_decode_frames
constexpr int RING = 128;               // restored samples kept in LDS: a chunk of 64 and the 32 before it

// a header that fails any check, its CRC-8 included, carries no block size that could be trusted: its frame takes no
// room in the output, and the frames behind it are placed behind the last good one
__device__ __forceinline__ bool hdr_parsed(int status) { return status == FHIP_VERIFY_OK; }

// ---- k_decode_frames -------------------------------------------------------------------------------

// SEG: the segment mode (DecodeArgs::seg_first): the strategy bit, the first number, continuity and the size rule of
// fixed blocks are a segment's; placement, pcm_cap, the records and the counts stay the batch's.  The carry across the
// chunks of DHDR_T frames is about frame f - 1 whatever its segment: a segment's first frame never looks at it.
//
// The window mode (on top of SEG): the scan S stays what it is -- the sizes of the good headers before the frame -- and
// gives the frame's place in its SEGMENT, S less S at the segment's head (kept in LDS for the chunk, carried across
// chunks for the one segment that can straddle a chunk's start: the one the last frame of the chunk before belongs to).
// The frame's clip against the segment's window follows; the scan of the clips' lengths is the frame's place in pcm, and
// pcm_cap, seg_start, seg_samples, nsamples and written_end are about the clips.
#if FHIP_K7_WINDOWS
#define K7_PLACE place      /* where the frame's delivered samples begin in pcm */
#define K7_SIZE cnt         /* how many it delivers */
__global__ void __launch_bounds__(DHDR_T) k_decode_frames_windows(DecodeWindowArgs w)
{
    constexpr bool SEG = true;
    const DecodeArgs &a = w.d;
    __shared__ long long s_S[DHDR_T];                  // S of each frame of the chunk
    __shared__ long long s_carry_head;                 // S at the head of the segment of the chunk's last frame
    if (threadIdx.x == 0) s_carry_head = 0;            // (first read behind the chunk loop's barriers)
    long long dbase = 0;
#else
#define K7_PLACE S
#define K7_SIZE h.n
template <bool SEG>
__global__ void __launch_bounds__(DHDR_T) k_decode_frames(DecodeArgs a)
{
#endif
    __shared__ long long scratch[DHDR_T / 64];
    __shared__ unsigned long long s_num[DHDR_T];      // the number and size each frame of the chunk carries
    __shared__ int s_n[DHDR_T];
    __shared__ int s_ok[DHDR_T];
    __shared__ unsigned long long s_carry_num;
    __shared__ int s_carry_n, s_carry_ok;
    __shared__ unsigned long long s_end;               // where the last frame that will be written ends
    const int count = a.nframes;
    const int t = threadIdx.x;
    VerifyArgs va{};                                   // what parse_header holds the codes against
    va.channels = a.channels;
    va.bps = a.bps;
    va.block_size = a.block_size;
    va.sample_rate = a.sample_rate;
    va.allow_vbs = a.variable_blocks;
    if (t == 0) {
        a.summary[0] = count;
        a.summary[1] = 0;
        a.key[0] = KEY_NONE;
        s_carry_num = 0;
        s_carry_n = 0;
        s_carry_ok = 0;
        s_end = 0;
    }
    if constexpr (SEG) {
        for (int s = t; s < a.nsegs; s += DHDR_T) { a.seg_samples[s] = 0; a.seg_failed[s] = -1; }
        __syncthreads();                               // (the sums below are atomic adds onto these zeros)
    }
    long long base = 0, sbase = 0, good = 0;
    for (int f0 = 0; f0 < count; f0 += DHDR_T) {
        const int f = f0 + t;
        const bool live = f < count;
        const long long fb = live ? (long long)a.frame_bytes[f] : 0;
        long long tot = 0;
        const long long off = base + block_excl_scan(fb > 0 ? fb : 0, scratch, DHDR_T / 64, &tot);
        base += tot;
        VerifyFrame vf{};
        vf.off = off;
        vf.bytes = (int)fb;
        HdrOut h{FHIP_VERIFY_OK, 0, 0, 0, 0, 0};
        // the frame's segment: the last one that starts at or before it (empty segments in front of it start there too)
        int seg = 0, variable = a.variable_blocks;
        bool seg_head = f == 0, seg_last = f == count - 1;
#if FHIP_K7_WINDOWS
        int head = 0;                                  // the first frame of the segment
#endif
        if constexpr (SEG) {
            if (live) {
                int lo = 0, hi = a.nsegs - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (a.seg_first[mid] <= f) lo = mid; else hi = mid - 1;
                }
                seg = lo;
                seg_head = a.seg_first[seg] == f;
#if FHIP_K7_WINDOWS
                head = a.seg_first[seg];
#endif
                seg_last = a.seg_first[seg + 1] == f + 1;
                variable = a.seg_variable[seg] != 0;
                va.allow_vbs = variable;
            }
        }
        if (live) {
            if (fb <= 0 || off + fb > a.stream_bytes) {
                h.status = FHIP_VERIFY_LENGTH;
                h.bit = fb <= 0 ? 0 : (a.stream_bytes - off) * 8;
                if (h.bit < 0) h.bit = 0;
            } else {
                h = parse_header(va, Bits{a.stream + off, fb});
            }
        }
        const bool parsed = live && hdr_parsed(h.status);
        s_num[t] = h.number;
        s_n[t] = h.n;
        s_ok[t] = parsed;
        __syncthreads();
        // frame f's first sample: the sizes the headers before it carry (a header that did not parse carries none)
        long long stot = 0;
        const long long S = sbase + block_excl_scan(parsed ? (long long)h.n : 0ll, scratch, DHDR_T / 64, &stot);
        sbase += stot;
#if FHIP_K7_WINDOWS
        // the frame's clip [lo, lo + cnt) of its own samples and where it goes (a header that did not parse: none)
        s_S[t] = S;
        __syncthreads();
        // (head <= f: inside the chunk or before it; a table that says otherwise reads nothing outside the chunk)
        const long long head_S = live && head >= f0 && head <= f ? s_S[head - f0] : s_carry_head;
        int lo = 0, cnt = 0;
        if (parsed) {
            const long long o = S - head_S;                                    // >= 0: S does not decrease
            const long long skip = w.seg_skip[seg] > 0 ? w.seg_skip[seg] : 0, take = w.seg_take[seg];
            const long long lim = (take < 0 || take > 0x7FFFFFFFFFFFFFFFll - skip) ? 0x7FFFFFFFFFFFFFFFll : skip + take;
            const long long c0 = o > skip ? o : skip, c1 = o + h.n < lim ? o + h.n : lim;
            if (c1 > c0) { lo = (int)(c0 - o); cnt = (int)(c1 - c0); }
        }
        long long dtot = 0;
        const long long place = dbase + block_excl_scan((long long)cnt, scratch, DHDR_T / 64, &dtot);
        dbase += dtot;
        __syncthreads();                                                       // (s_carry_head has been read by everyone)
        if (t == DHDR_T - 1) s_carry_head = head_S;
#endif
        if (live && h.status == FHIP_VERIFY_OK) {
            // (a frame whose own header is broken has already failed: its successor is not blamed for it)
            const unsigned long long prev_num = t ? s_num[t - 1] : s_carry_num;
            const int prev_n = t ? s_n[t - 1] : s_carry_n;
            const bool prev_ok = !seg_head && (t ? s_ok[t - 1] : s_carry_ok);
            unsigned long long want = h.number;
            if (seg_head) {
                const long long first = SEG ? a.seg_number[seg] : a.first_number;
                if (first >= 0) want = (unsigned long long)first;
            } else if (prev_ok) {
                want = prev_num + (variable ? (unsigned long long)prev_n : 1ull);
            }
            // fixed blocks: every frame but the last holds the same number of samples
            bool size_ok = true;
            if (!variable && prev_ok) size_ok = seg_last ? h.n <= prev_n : h.n == prev_n;
            const bool fits = K7_PLACE + K7_SIZE <= a.pcm_cap;      // (windows: a frame that delivers nothing fits, below)
            if (h.number != want) { h.status = FHIP_VERIFY_NUMBER; h.bit = 32; }
#if FHIP_K7_WINDOWS
            else if (!size_ok || (!fits && cnt > 0)) { h.status = FHIP_VERIFY_NUMBER; h.bit = 16; }
#else
            else if (!size_ok || !fits) { h.status = FHIP_VERIFY_NUMBER; h.bit = 16; }
#endif
        }
        long long gtot = 0;
        const long long G = good + block_excl_scan(live && h.status == FHIP_VERIFY_OK ? (long long)K7_SIZE : 0ll, scratch,
                                                   DHDR_T / 64, &gtot);
        good += gtot;
        if constexpr (SEG) {
            if (live && seg_head) {
                // the segment begins at S, and G good samples lie before it: they end the count of the last segment
                // with a frame and start this one's (two adds per segment, in any order).  Empty segments in front
                // of this frame begin here as well.
                a.seg_start[seg] = K7_PLACE;
                atomicAdd((unsigned long long *)&a.seg_samples[seg], (unsigned long long)-G);
                int sp = seg - 1;
                for (; sp >= 0 && a.seg_first[sp] == f; sp--) a.seg_start[sp] = K7_PLACE;
                if (sp >= 0) atomicAdd((unsigned long long *)&a.seg_samples[sp], (unsigned long long)G);
            }
        }
#if FHIP_K7_WINDOWS
        if (live && h.status == FHIP_VERIFY_OK && cnt > 0) atomicMax(&s_end, (unsigned long long)(place + cnt));
        if (live) w.clip[f] = DecodeClip{place, lo, h.status == FHIP_VERIFY_OK ? cnt : 0};
#else
        if (live && h.status == FHIP_VERIFY_OK) atomicMax(&s_end, (unsigned long long)(S + h.n));
#endif
        if (live) {
            vf.rel_start = K7_PLACE;
            vf.n = h.n;
            vf.hdr_bits = h.hdr_bits;
            vf.ch_code = h.ch_code;
            vf.status = h.status;
            vf.bit = h.bit;
            a.ws[f] = vf;
        }
        __syncthreads();
        if (t == DHDR_T - 1) { s_carry_num = s_num[t]; s_carry_n = s_n[t]; s_carry_ok = s_ok[t]; }
        __syncthreads();
    }
    if (t == 0) {
        a.nsamples[0] = good;
        a.written_end[0] = (long long)s_end;
        if constexpr (SEG) {
            // segments behind the last frame are empty and begin at the batch's end; the last one with a frame ends there
            int sp = a.nsegs - 1;
#if FHIP_K7_WINDOWS
            for (; sp >= 0 && a.seg_first[sp] == count; sp--) a.seg_start[sp] = dbase;
#else
            for (; sp >= 0 && a.seg_first[sp] == count; sp--) a.seg_start[sp] = sbase;
#endif
            if (sp >= 0) atomicAdd((unsigned long long *)&a.seg_samples[sp], (unsigned long long)good);
        }
    }
}

// ---- k_decode --------------------------------------------------------------------------------------

// a raw signed field of w bits, 1 .. 33; a 33-bit field (the side channel of a 32-bit stream) is read wrapped
// to int32, as the verifier reads it: only its low 32 bits carry the value
__device__ __forceinline__ int32_t rd_signed(const Bits &bs, long long p, int w)
{
    if (w <= 0) return 0;
    if (w > 32) { p += w - 32; w = 32; }
    uint32_t v = bs.rd(p, w);
    if (w < 32 && (v & (1u << (w - 1)))) v |= ~((1u << w) - 1u);
    return (int32_t)v;
}

// The window mode: the frame's clip (DecodeClip, left by the header pass) replaces [rel_start, rel_start + n) in the
// write-out; everything before it is the same code.
#if FHIP_K7_WINDOWS
__global__ void __launch_bounds__(DT) k_decode_windows(DecodeWindowArgs w)
{
    const DecodeArgs &a = w.d;
#else
__global__ void __launch_bounds__(DT) k_decode(DecodeArgs a)
{
#endif
    __shared__ uint8_t fb_lds[DFB_CAP];
    __shared__ int32_t ybuf[RING];
    __shared__ SubHdr s_sh;
    __shared__ int s_wasted[FHIP_MAX_CH];
    __shared__ unsigned long long s_key;
    __shared__ long long s_pos;
    __shared__ uint32_t s_crc;

    const int f = blockIdx.x, lane = threadIdx.x;
    const VerifyFrame vf = a.ws[f];
    unsigned long long key = KEY_NONE;
    if (vf.status != FHIP_VERIFY_OK) {
        key = mkkey(vf.bit, 15, 0xFFFF, vf.status);
    } else {
        // stage the frame (pass 1 put it inside the stream)
        const uint8_t *src = a.stream + vf.off;
        const bool staged = vf.bytes <= DFB_CAP;
        if (staged)
            for (int i = lane; i < vf.bytes; i += DT) fb_lds[i] = src[i];
        const Bits bs{staged ? fb_lds : src, vf.bytes};
        const long long end = (long long)vf.bytes * 8;
        const int n = vf.n;                              // 1 .. block_size (parse_header)
        const int nch = a.channels;
        int32_t *const rows = a.rows + (size_t)f * (size_t)nch * (size_t)a.block_size;
        if (lane == 0) { s_key = KEY_NONE; s_pos = vf.hdr_bits; }
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            __syncthreads();                   // everybody is done with the previous subframe's shared state
            const bool side = (vf.ch_code == FHIP_CH_LEFT_SIDE && c == 1) || (vf.ch_code == FHIP_CH_RIGHT_SIDE && c == 0) ||
                              (vf.ch_code == FHIP_CH_MID_SIDE && c == 1);
            const int sub_bps = a.bps + (side ? 1 : 0);
            if (lane == 0) {
                const unsigned long long k = parse_subframe(bs, s_pos, end, sub_bps, n, &s_sh, c);
                if (k != KEY_NONE) s_key = k;
                else s_wasted[c] = s_sh.wasted;
            }
            __syncthreads();
            if (s_key != KEY_NONE) break;
            const SubHdr &sh = s_sh;
            int32_t *const row = rows + (size_t)c * (size_t)a.block_size;
            const int w = sh.w;
            if (sh.type == FHIP_SUB_CONSTANT || sh.type == FHIP_SUB_VERBATIM) {
                const bool constant = sh.type == FHIP_SUB_CONSTANT;
                const long long sub_end = sh.pos + (constant ? (long long)w : (long long)n * w);
                if (sub_end > end) {
                    if (lane == 0) s_key = mkkey(end, c, 0xFFFF, FHIP_VERIFY_SYNTAX);
                } else {
                    for (int i = lane; i < n; i += DT) row[i] = rd_signed(bs, sh.pos + (constant ? 0ll : (long long)i * w), w);
                    if (lane == 0) s_pos = sub_end;
                }
            } else {
                const int order = sh.order;                  // <= n, <= 32; the warm-up lies inside the frame (parse_subframe)
                if (lane < order) {
                    const int32_t v = rd_signed(bs, sh.pos + (long long)lane * w, w);
                    row[lane] = v;
                    ybuf[lane & (RING - 1)] = v;
                }
                __syncthreads();
                // lane 0's walk: the partition it is in, the residuals left in it, the bit position
                const int npart = 1 << sh.porder, psz = n >> sh.porder;
                const int pbits = sh.method ? 5 : 4, escv = sh.method ? 31 : 15;
                const bool lpc = sh.type == FHIP_SUB_LPC;
                const int shift = sh.shift;
                long long p = sh.res + 6;
                int part = -1, left = 0, k = 0;
                bool esc = false;
                unsigned long long wkey = KEY_NONE;
#define WFAIL() do { wkey = mkkey(end, c, 0xFFFF, FHIP_VERIFY_SYNTAX); } while (0)
                // the next partition's parameter (and raw width); false: it lies past the frame's end
                auto next_partition = [&]() -> bool {
                    part++;
                    if (p + pbits > end) return false;
                    k = (int)bs.rd(p, pbits);
                    p += pbits;
                    esc = k == escv;
                    if (esc) {
                        if (p + 5 > end) return false;
                        k = (int)bs.rd(p, 5);
                        p += 5;
                    }
                    left = psz - (part == 0 ? order : 0);
                    return true;
                };
                for (int i0 = order; i0 < n; i0 += DT) {
                    const int i1 = min(i0 + DT, n);
                    if (lane == 0 && wkey == KEY_NONE) {
                        for (int i = i0; i < i1; i++) {
                            // (the partitions hold n - order residuals in all: part stays below npart)
                            while (left == 0 && wkey == KEY_NONE)
                                if (!next_partition()) WFAIL();
                            if (wkey != KEY_NONE) break;
                            int32_t e;
                            if (esc) {
                                if (p + k > end) { WFAIL(); break; }
                                e = rd_signed(bs, p, k);
                                p += k;
                            } else {
                                uint32_t q = 0;
                                for (;;) {
                                    if (p >= end) { WFAIL(); break; }
                                    const int take = end - p < 32 ? (int)(end - p) : 32;
                                    const uint32_t v = bs.rd(p, take);
                                    if (v) {
                                        const int z = __clz(v) - (32 - take);
                                        q += (uint32_t)z;
                                        p += z + 1;
                                        break;
                                    }
                                    q += (uint32_t)take;
                                    p += take;
                                }
                                if (wkey != KEY_NONE) break;
                                if (p + k > end) { WFAIL(); break; }
                                const uint32_t u = (q << k) | bs.rd(p, k);
                                p += k;
                                e = (int32_t)(u >> 1) ^ -(int32_t)(u & 1u);
                            }
                            left--;
                            // the prediction: a 64-bit sum, an arithmetic shift; the sample wrapped to int32
                            long long pred = 0;
                            if (lpc) {
                                long long acc = 0;
                                for (int j = 0; j < order; j++) acc += (long long)sh.coef[j] * (long long)ybuf[(i - 1 - j) & (RING - 1)];
                                pred = acc >> shift;
                            } else {
#define Y(d) ((long long)ybuf[(i - (d)) & (RING - 1)])
                                switch (order) {
                                case 1: pred = Y(1); break;
                                case 2: pred = 2 * Y(1) - Y(2); break;
                                case 3: pred = 3 * Y(1) - 3 * Y(2) + Y(3); break;
                                case 4: pred = 4 * Y(1) - 6 * Y(2) + 4 * Y(3) - Y(4); break;
                                default: break;
                                }
#undef Y
                            }
                            ybuf[i & (RING - 1)] = (int32_t)(uint32_t)((uint64_t)(long long)e + (uint64_t)pred);
                        }
                    }
                    __syncthreads();
                    const int i = i0 + lane;
                    if (i < i1) row[i] = ybuf[i & (RING - 1)];       // (past a failed read: unspecified, the frame fails)
                    __syncthreads();
                }
                if (lane == 0) {
                    // partitions without a residual still carry their parameter (n == order; psz == order)
                    while (wkey == KEY_NONE && part < npart - 1)
                        if (!next_partition()) WFAIL();
                    if (wkey != KEY_NONE) s_key = wkey;
                    s_pos = p;
                }
#undef WFAIL
            }
            __syncthreads();
            if (s_key != KEY_NONE) break;
        }
        // padding to the byte, CRC-16, the end
        __syncthreads();
        const bool clean = s_key == KEY_NONE;
        __syncthreads();
        if (clean) {
            const long long p = s_pos;
            const long long body = (p + 7) >> 3;                      // bytes the CRC-16 covers
            if (lane == 0) {
                unsigned long long k = KEY_NONE;
                if (p > end) k = mkkey(end, 15, 0xFFFF, FHIP_VERIFY_SYNTAX);
                else if (body * 8 > p && bs.rd(p, (int)(body * 8 - p)) != 0) {
                    const int nb = (int)(body * 8 - p);
                    const uint32_t v = bs.rd(p, nb);
                    k = mkkey(p + (__clz(v) - (32 - nb)), 15, 0xFFFF, FHIP_VERIFY_PADDING);
                } else if (body + 2 > vf.bytes) {
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
                const long long L = (body + DT - 1) / DT;
                const long long b0 = (long long)lane * L, b1 = min(b0 + L, body);
                uint32_t crc = 0;
                for (long long i = b0; i < b1; i++) crc = crc16_byte(crc, bs.byte(i));
                if (b0 < b1 && crc) crc = gf16_mul(crc, gf16_xpow8(body - b1));
                for (int d = 32; d > 0; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
                if (lane == 0) {
                    const uint32_t got = bs.rd(body * 8, 16);
                    if (got != crc) s_key = mkkey(body * 8, 15, 0xFFFF, FHIP_VERIFY_CRC16);
                    else if (body + 2 != vf.bytes) s_key = mkkey((body + 2) * 8, 15, 0xFFFF, FHIP_VERIFY_LENGTH);
                }
            }
        }
        __syncthreads();
        key = s_key;
        if (key == KEY_NONE) {
            // the frame passed: wasted-bit shift, channel recombination, interleave.  k_decode_frames placed
            // [rel_start, rel_start + n) inside [0, pcm_cap)
#if FHIP_K7_WINDOWS
            // the clip [lo, lo + cnt) of the frame goes to [dst, dst + cnt): i runs over the clip alone, inside the frame
            // whatever the table holds, and g = dst + (i - lo)
            const DecodeClip cl = w.clip[f];
            const long long S = cl.dst - cl.lo;
            const int i0 = max(cl.lo, 0), i1 = min(cl.lo + cl.cnt, n);
#else
            const long long S = vf.rel_start;
            const int i0 = 0, i1 = n;
#endif
            int16_t *const out16 = reinterpret_cast<int16_t *>(a.pcm);
            int32_t *const out32 = reinterpret_cast<int32_t *>(a.pcm);
            const bool s16 = a.pcm_format == FHIP_PCM_S16;
            for (int i = i0 + lane; i < i1; i += DT) {
                const long long g = S + i;
                if (g < 0 || g >= a.pcm_cap) continue;
                if (vf.ch_code >= 8) {
                    const int32_t v0 = (int32_t)((uint32_t)rows[i] << s_wasted[0]);
                    const int32_t v1 = (int32_t)((uint32_t)rows[(size_t)a.block_size + i] << s_wasted[1]);
                    int32_t l, r;
                    if (vf.ch_code == FHIP_CH_LEFT_SIDE) {
                        l = v0;
                        r = (int32_t)((uint32_t)v0 - (uint32_t)v1);
                    } else if (vf.ch_code == FHIP_CH_RIGHT_SIDE) {
                        r = v1;
                        l = (int32_t)((uint32_t)v0 + (uint32_t)v1);
                    } else {
                        const long long mid = ((long long)v0 << 1) | (long long)(v1 & 1), sd = v1;
                        l = (int32_t)((mid + sd) >> 1);
                        r = (int32_t)((mid - sd) >> 1);
                    }
                    if (s16) { out16[g * 2] = (int16_t)l; out16[g * 2 + 1] = (int16_t)r; }
                    else { out32[g * 2] = l; out32[g * 2 + 1] = r; }
                } else {
                    for (int c = 0; c < nch; c++) {
                        const int32_t v = (int32_t)((uint32_t)rows[(size_t)c * (size_t)a.block_size + i] << s_wasted[c]);
                        if (s16) out16[g * nch + c] = (int16_t)v;
                        else out32[g * nch + c] = v;
                    }
                }
            }
        }
    }
    if (lane == 0) {
        const int status = key == KEY_NONE ? FHIP_VERIFY_OK : (int)(key & 15);
        if (a.recs) {
            fhip_verify_rec r;
            r.status = status;
            r.bit = status == FHIP_VERIFY_OK ? -1 : (int32_t)min((long long)(key >> 24), 0x7FFFFFFFll);
            const int sub = (int)((key >> 20) & 15);
            r.subframe = (status == FHIP_VERIFY_OK || sub == 15) ? -1 : sub;
            r.sample = -1;
            a.recs[f] = r;
        }
        if (status != FHIP_VERIFY_OK) {
            atomicAdd((unsigned long long *)&a.summary[1], 1ull);
            atomicMin(&a.key[0], ((unsigned long long)f << 8) | (unsigned long long)status);
        }
    }
}

#if !FHIP_K7_WINDOWS
__global__ void k_decode_final(DecodeArgs a)
{
    const unsigned long long k = a.key[0];
    a.summary[2] = k == KEY_NONE ? -1 : (long long)(k >> 8);
    a.summary[3] = k == KEY_NONE ? 0 : (long long)(k & 0xFF);
}

// The segment mode's end: seg_failed[s] = the first frame of segment s whose record k_decode left with a status (the
// header pass's failures went through k_decode into the records like every other).  A wave per segment, 64 frames a step.
__global__ void __launch_bounds__(DT) k_decode_seg_final(DecodeArgs a)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const int f0 = max(a.seg_first[s], 0), f1 = min(a.seg_first[s + 1], a.nframes);    // (never past the records)
    for (int fb = f0; fb < f1; fb += DT) {
        const int f = fb + lane;
        const bool bad = f < f1 && a.recs[f].status != FHIP_VERIFY_OK;
        const unsigned long long m = __ballot(bad);
        if (m) {                                          // wave-uniform
            if (lane == 0) a.seg_failed[s] = fb + __ffsll(m) - 1;
            return;
        }
    }
}

#endif

}  // namespace

#if FHIP_K7_WINDOWS
hipError_t launch_decode_windows(hipStream_t st, const DecodeWindowArgs &w)
{
    const DecodeArgs &a = w.d;
    if (!a.seg_first || a.nsegs < 1 || !a.seg_number || !a.seg_variable || !a.seg_start || !a.seg_samples || !a.seg_failed ||
        !w.seg_skip || !w.seg_take || (a.nframes > 0 && (!a.recs || !w.clip)))
        return hipErrorInvalidValue;
    note_launch("k_decode_frames windows");
    hipLaunchKernelGGL(k_decode_frames_windows, dim3(1), dim3(DHDR_T), 0, st, w);
    if (a.nframes > 0) {
        note_launch("k_decode windows");
        hipLaunchKernelGGL(k_decode_windows, dim3(a.nframes), dim3(DT), 0, st, w);
    }
    return launch_decode_end(st, a);
}
#else
hipError_t launch_decode_end(hipStream_t st, const DecodeArgs &a)
{
    note_launch("k_decode_final");
    hipLaunchKernelGGL(k_decode_final, dim3(1), dim3(1), 0, st, a);
    if (a.seg_first && a.nframes > 0) {
        note_launch("k_decode_seg_final");
        hipLaunchKernelGGL(k_decode_seg_final, dim3(a.nsegs), dim3(DT), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_decode(hipStream_t st, const DecodeArgs &a)
{
    const bool seg = a.seg_first != nullptr;
    if (seg) {
        if (a.nsegs < 1 || !a.seg_number || !a.seg_variable || !a.seg_start || !a.seg_samples || !a.seg_failed ||
            (a.nframes > 0 && !a.recs))
            return hipErrorInvalidValue;
        note_launch("k_decode_frames segments");
        hipLaunchKernelGGL(k_decode_frames<true>, dim3(1), dim3(DHDR_T), 0, st, a);
    } else {
        note_launch("k_decode_frames");
        hipLaunchKernelGGL(k_decode_frames<false>, dim3(1), dim3(DHDR_T), 0, st, a);
    }
    if (a.nframes > 0) {
        note_launch("k_decode");
        hipLaunchKernelGGL(k_decode, dim3(a.nframes), dim3(DT), 0, st, a);
    }
    return launch_decode_end(st, a);
}
#endif

}  // namespace fhip
