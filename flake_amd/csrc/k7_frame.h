// k7_frame.h -- K7's two passes, written once for every mode: the header pass decode_frames<SEG, WIN> and the window mode's
// frame pass decode_frame_window.  k7_decode.hip and k7_decode_windows.hip make their kernels of them, each kernel a wrapper that
// names its instance.  What a mode adds is under if constexpr, so an instance carries nothing of the modes it is not:
// the register and LDS figures of the kernels are pinned by tests.
// SEG, the segment mode (DecodeArgs::seg_first): the strategy bit, the first number, continuity and the size rule of
// fixed blocks are a segment's; placement, pcm_cap, the records and the counts stay the batch's.
// WIN, the window mode (on top of SEG; DecodeWindowArgs): segment s delivers only samples [seg_skip[s], seg_skip[s] +
// seg_take[s]) of its own, counted over the sizes of its good headers.  Every frame is still parsed, restored and
// checked in full; what changes is where a frame's samples go and which of them: the header pass leaves a DecodeClip per
// frame, and the write-out of the frame pass runs over the clip alone.
#pragma once

#include "flac_frame_pass.h"

namespace fhip {
namespace {

constexpr int DT = 64;                  // lanes per frame: one wave
constexpr int DFB_CAP = 16384;          // frames up to this many bytes are staged in LDS
constexpr int DHDR_T = 1024;            // lanes of the header pass
constexpr int RING = 128;               // restored samples kept in LDS: a chunk of 64 and the 32 before it

// a header that fails any check, its CRC-8 included, carries no block size that could be trusted: its frame takes no
// room in the output, and the frames behind it are placed behind the last good one
__device__ __forceinline__ bool hdr_parsed(int status) { return status == FHIP_VERIFY_OK; }

// the tables of the segment mode, as both launchers need them (windows: the window tables and the clips on top)
inline bool decode_segments_ok(const DecodeArgs &a)
{
    return a.seg_first && a.nsegs >= 1 && a.seg_number && a.seg_variable && a.seg_start && a.seg_samples && a.seg_failed &&
           (a.nframes == 0 || a.recs);
}

// ---- the header pass --------------------------------------------------------------------------------

// the window mode's LDS; nothing in the other instances
template <bool WIN> struct WindowScan {};
template <> struct WindowScan<true> {
    long long S[DHDR_T];                // S of each frame of the chunk
    long long carry_head;               // S at the head of the segment of the chunk's last frame
};

// One workgroup of DHDR_T lanes, a frame per lane and chunk.  The carry across the chunks is about frame f - 1 whatever
// its segment: a segment's first frame never looks at it.
//
// WIN: the scan S stays what it is -- the sizes of the good headers before the frame -- and gives the frame's place in
// its SEGMENT, S less S at the segment's head (kept in LDS for the chunk, carried across chunks for the one segment that
// can straddle a chunk's start: the one the last frame of the chunk before belongs to).  The frame's clip against the
// segment's window follows; the scan of the clips' lengths is the frame's place in pcm, and pcm_cap, seg_start,
// seg_samples, nsamples and written_end are about the clips.  w is null in the other instances.
template <bool SEG, bool WIN>
__device__ __forceinline__ void decode_frames(const DecodeArgs &a, const DecodeWindowArgs *w)
{
    static_assert(SEG || !WIN, "the window mode is a segment mode");
    __shared__ long long scratch[DHDR_T / 64];
    __shared__ unsigned long long s_num[DHDR_T];      // the number and size each frame of the chunk carries
    __shared__ int s_n[DHDR_T];
    __shared__ int s_ok[DHDR_T];
    __shared__ unsigned long long s_carry_num;
    __shared__ int s_carry_n, s_carry_ok;
    __shared__ unsigned long long s_end;               // where the last frame that will be written ends
    __shared__ WindowScan<WIN> s_win;
    const int count = a.nframes;
    const int t = threadIdx.x;
    VerifyArgs va{};                                   // what frame_header reads: the stream, the codes' yardsticks
    va.stream = a.stream;
    va.stream_bytes = a.stream_bytes;
    va.frame_bytes = a.frame_bytes;
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
        if constexpr (WIN) s_win.carry_head = 0;       // (first read behind the chunk loop's barriers)
    }
    if constexpr (SEG) {
        for (int s = t; s < a.nsegs; s += DHDR_T) { a.seg_samples[s] = 0; a.seg_failed[s] = -1; }
        __syncthreads();                               // (the sums below are atomic adds onto these zeros)
    }
    long long base = 0, sbase = 0, good = 0, dbase = 0;      // (dbase, WIN: the clips' lengths so far)
    for (int f0 = 0; f0 < count; f0 += DHDR_T) {
        const int f = f0 + t;
        const bool live = f < count;
        // the frame's segment: the last one that starts at or before it (empty segments in front of it start there too)
        int seg = 0, variable = a.variable_blocks;
        bool seg_head = f == 0, seg_last = f == count - 1;
        int head = 0;                                  // WIN: the first frame of the segment
        if constexpr (SEG) {
            if (live) {
                int lo = 0, hi = a.nsegs - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (a.seg_first[mid] <= f) lo = mid; else hi = mid - 1;
                }
                seg = lo;
                seg_head = a.seg_first[seg] == f;
                if constexpr (WIN) head = a.seg_first[seg];
                seg_last = a.seg_first[seg + 1] == f + 1;
                variable = a.seg_variable[seg] != 0;
                va.allow_vbs = variable;
            }
        }
        VerifyFrame vf{};
        HdrOut h = frame_header<DHDR_T>(va, f, live, base, scratch, vf);
        const bool parsed = live && hdr_parsed(h.status);
        s_num[t] = h.number;
        s_n[t] = h.n;
        s_ok[t] = parsed;
        __syncthreads();
        // frame f's first sample: the sizes the headers before it carry (a header that did not parse carries none)
        long long stot = 0;
        const long long S = sbase + block_excl_scan(parsed ? (long long)h.n : 0ll, scratch, DHDR_T / 64, &stot);
        sbase += stot;
        long long place = S;                           // where the frame's delivered samples begin in pcm
        int lo = 0, cnt = h.n;                         // its clip [lo, lo + cnt): all (a header that did not parse: n = 0)
        if constexpr (WIN) {
            s_win.S[t] = S;
            __syncthreads();
            // (head <= f: inside the chunk or before it; a table that says otherwise reads nothing outside the chunk)
            const long long head_S = live && head >= f0 && head <= f ? s_win.S[head - f0] : s_win.carry_head;
            cnt = 0;
            if (parsed) {
                const long long o = S - head_S;                                    // >= 0: S does not decrease
                const long long skip = w->seg_skip[seg] > 0 ? w->seg_skip[seg] : 0, take = w->seg_take[seg];
                const long long lim = (take < 0 || take > 0x7FFFFFFFFFFFFFFFll - skip) ? 0x7FFFFFFFFFFFFFFFll : skip + take;
                const long long c0 = o > skip ? o : skip, c1 = o + h.n < lim ? o + h.n : lim;
                if (c1 > c0) { lo = (int)(c0 - o); cnt = (int)(c1 - c0); }
            }
            long long dtot = 0;
            place = dbase + block_excl_scan((long long)cnt, scratch, DHDR_T / 64, &dtot);
            dbase += dtot;
            __syncthreads();                                                       // (carry_head has been read by everyone)
            if (t == DHDR_T - 1) s_win.carry_head = head_S;
        }
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
            // (windows: a frame that delivers nothing fits)
            const bool fits = place + cnt <= a.pcm_cap || (WIN && cnt == 0);
            if (h.number != want) { h.status = FHIP_VERIFY_NUMBER; h.bit = 32; }
            else if (!size_ok || !fits) { h.status = FHIP_VERIFY_NUMBER; h.bit = 16; }
        }
        const bool good_frame = live && h.status == FHIP_VERIFY_OK;
        long long gtot = 0;
        const long long G = good + block_excl_scan(good_frame ? (long long)cnt : 0ll, scratch, DHDR_T / 64, &gtot);
        good += gtot;
        if constexpr (SEG) {
            if (live && seg_head) {
                // the segment begins at place, and G good samples lie before it: they end the count of the last segment
                // with a frame and start this one's (two adds per segment, in any order).  Empty segments in front
                // of this frame begin here as well.
                a.seg_start[seg] = place;
                atomicAdd((unsigned long long *)&a.seg_samples[seg], (unsigned long long)-G);
                int sp = seg - 1;
                for (; sp >= 0 && a.seg_first[sp] == f; sp--) a.seg_start[sp] = place;
                if (sp >= 0) atomicAdd((unsigned long long *)&a.seg_samples[sp], (unsigned long long)G);
            }
        }
        if (good_frame && (!WIN || cnt > 0)) atomicMax(&s_end, (unsigned long long)(place + cnt));
        if constexpr (WIN)
            if (live) w->clip[f] = DecodeClip{place, lo, good_frame ? cnt : 0};
        if (live) {
            vf.rel_start = place;
            frame_fill(vf, h);
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
            const long long batch_end = WIN ? dbase : sbase;
            int sp = a.nsegs - 1;
            for (; sp >= 0 && a.seg_first[sp] == count; sp--) a.seg_start[sp] = batch_end;
            if (sp >= 0) atomicAdd((unsigned long long *)&a.seg_samples[sp], (unsigned long long)good);
        }
    }
}

// ---- the frame pass ---------------------------------------------------------------------------------

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

// The window mode's frame pass, one wave per frame: k7_decode.hip's k_decode in which the frame's clip (clip[f], left by
// the header pass) replaces [rel_start, rel_start + n) in the write-out.  (k_decode keeps its text in its kernel: as an
// instance of this function it ran 2 to 4 % slower, profiles/k5_k7_frame_pass_refactor.txt.  A change to the walk goes
// into both.)
__device__ __forceinline__ void decode_frame_window(const DecodeArgs &a, const DecodeClip *clip)
{
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
        const Bits bs = frame_stage<DT>(fb_lds, a.stream + vf.off, vf.bytes);
        const long long end = (long long)vf.bytes * 8;
        const int n = vf.n;                              // 1 .. block_size (parse_header)
        const int nch = a.channels;
        int32_t *const rows = a.rows + (size_t)f * (size_t)nch * (size_t)a.block_size;
        if (lane == 0) { s_key = KEY_NONE; s_pos = vf.hdr_bits; }
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            __syncthreads();                   // everybody is done with the previous subframe's shared state
            const int sub_bps = subframe_bps(a.bps, vf.ch_code, c);
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
        __syncthreads();
        key = frame_tail<DT>(bs, vf.bytes, s_key, s_pos, s_crc);
        if (key == KEY_NONE) {
            // the frame passed: wasted-bit shift, channel recombination, interleave.  The header pass placed
            // [rel_start, rel_start + n) inside [0, pcm_cap)
            // the clip [lo, lo + cnt) of the frame goes to [dst, dst + cnt): i runs over the clip alone, inside the frame
            // whatever the table holds, and g = dst + (i - lo)
            const DecodeClip cl = clip[f];
            const long long S = cl.dst - cl.lo;
            const int i0 = max(cl.lo, 0), i1 = min(cl.lo + cl.cnt, n);
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
    if (lane == 0) frame_record<false>(a.recs, a.summary, a.key, f, key);
}

}  // namespace
}  // namespace fhip
