// k7_decode.hip -- K7: FLAC frames back to PCM.
//
// The inverse of the encode path, by the FLAC format alone: a batch of frames whose byte sizes are known is
// parsed, its residuals are read, the prediction recurrence runs and the channel transform is undone.  Laid out
// like K5 (k5_verify.hip), with which it shares the bit reader and the header parsers (flac_parse.h) and the header
// pass's prologue (flac_frame_pass.h):
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
// The header pass is k7_frame.h's decode_frames<SEG, WIN>, of which k_decode_frames<SEG> are the instances without a
// window.  k_decode keeps its text in the kernel itself: as an instance of a shared inline body, or with
// flac_frame_pass.h's pieces in it, it ran 2 to 4 % slower (profiles/k5_k7_frame_pass_refactor.txt).  Its window twin is
// k7_frame.h's decode_frame_window: a change to the frame pass goes into both.
#include "k7_frame.h"

namespace fhip {
namespace {

template <bool SEG>
__global__ void __launch_bounds__(DHDR_T) k_decode_frames(DecodeArgs a) { decode_frames<SEG, false>(a, nullptr); }

__global__ void __launch_bounds__(DT) k_decode(DecodeArgs a)
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
            // the frame passed: wasted-bit shift, channel recombination, interleave.  The header pass placed
            // [rel_start, rel_start + n) inside [0, pcm_cap)
            const long long S = vf.rel_start;
            const int i0 = 0, i1 = n;
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

__global__ void k_decode_final(DecodeArgs a) { frame_summary_end(a.key[0], a.summary); }

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

}  // namespace

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
        if (!decode_segments_ok(a)) return hipErrorInvalidValue;
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

}  // namespace fhip
