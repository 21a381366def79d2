// k11_held.hip -- K11: what a corpus that stays on the device needs in front of K7.  Two small stages, both on tables of
// frames that lie anywhere in a resident store of FLAC bytes:
//
//   k_frame_heads      one lane per frame: flac_header_ok (flac_header.h, the one predicate every reader shares) on the
//                      frame's first bytes, its answer in a 16-byte record.  The host keeps the records and selects
//                      windows over them without parsing a stream byte again.
//   k_frame_offsets    a wave per range: where each frame K8 found begins -- its range's first byte plus the sizes of the
//                      range's frames before it -- so that k_frame_heads can follow K8 with no host step in between.
//   k_gather_offsets   one workgroup: which frames of a list are accepted (a length of at least 1, a source range inside
//   k_gather_frames    the store, a place that fits the destination) and where each lands -- the exclusive prefix sum of
//                      the accepted lengths before it; then a wave per frame copies it there.  The result is the
//                      contiguous stream and the frame_bytes table that K7 takes.
//
// Memory safety is structural, as K7's, K8's and K9's: a header is read inside its frame's range and inside the stream,
// a source byte inside [0, src_bytes), a destination byte inside the frame's own range and inside [0, dst_cap) --
// whatever the device tables hold.  k_gather_frames holds every frame against those bounds again instead of trusting
// what k_gather_offsets left.
//
// The copy: the bytes before the destination's first 16-byte boundary and behind its last go lane by lane; between
// them a lane stores 16 aligned bytes at a time, loaded in one piece where the source agrees with the destination
// modulo 16 and byte by byte where it does not (K9's rule for disagreeing residues).  No load ever covers a byte that
// is not the frame's, so the store's first and last byte may be the allocation's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace fhip {
namespace {

constexpr int HEADS_T = 256;
constexpr int SCAN_T = 1024;                                    // k_gather_offsets: frames per round of its one workgroup
constexpr int SCAN_WAVES = SCAN_T / 64;
constexpr int COPY_T = 256;                                     // k_gather_frames: a wave per frame
constexpr int COPY_FRAMES = COPY_T / 64;

__global__ __launch_bounds__(HEADS_T) void k_frame_heads(FrameHeadsArgs a)
{
    const long long f = (long long)blockIdx.x * HEADS_T + threadIdx.x;
    if (f >= a.nframes) return;
    const long long off = a.frame_off[f], fb = a.frame_bytes[f];
    fhip_frame_head r;
    r.number = 0;
    r.n = 0;
    r.flags = 0;
    flac_header h;
    if (fb > 0 && off >= 0 && off <= a.stream_bytes - fb && flac_header_ok(&a.fmt, a.stream + off, fb, &h)) {
        r.number = h.number;
        r.n = h.n;
        r.flags = 1 | (h.vbs ? 2 : 0) | ((h.len & 0xFF) << 8);
    }
    a.heads[f] = r;
}

// K8 leaves the sizes of all ranges' frames back to back in range order and each range's count (below 0: refused, no
// frames).  Range r's first frame is the counts before it added up; its frames lie back to back from range_first[r] on.
__global__ __launch_bounds__(HEADS_T) void k_frame_offsets(FrameOffsetsArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (HEADS_T / 64) + (threadIdx.x >> 6);
    if (r >= a.nranges) return;
    long long first = 0;
    for (long long q = lane; q < r; q += 64) {
        const int n = a.range_frames[q];
        first += n > 0 ? n : 0;
    }
    for (int d = 32; d; d >>= 1) first += __shfl_xor(first, d);
    const int nf = a.range_frames[r];
    long long at = a.base + a.range_first[r];
    for (int k0 = 0; k0 < nf; k0 += 64) {
        const long long f = first + k0 + lane;
        const bool mine = k0 + lane < nf && f < a.frame_cap;
        const long long len = mine ? a.frame_bytes[f] : 0;
        long long inc = len;
        for (int d = 1; d < 64; d <<= 1) {
            const long long v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (mine) a.frame_off[f] = at + inc - len;
        at += __shfl(inc, 63);
    }
}

// The length frame f is copied with, as far as the source decides: 0 where the frame is not one to copy.
__device__ inline long long source_len(const GatherFramesArgs &a, int f)
{
    const long long s = a.frame_src[f], l = a.frame_len[f];
    return l >= 1 && s >= 0 && s <= a.src_bytes - l ? l : 0;
}

__global__ __launch_bounds__(SCAN_T) void k_gather_offsets(GatherFramesArgs a)
{
    __shared__ long long wtot[SCAN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;                                        // the accepted bytes before this round (uniform)
    for (int base = 0; base < a.nframes; base += SCAN_T) {
        const int f = base + (int)threadIdx.x;
        const long long len = f < a.nframes ? source_len(a, f) : 0;
        long long inc = len;
        for (int d = 1; d < 64; d <<= 1) {
            const long long v = __shfl_up(inc, d);
            if (lane >= d) inc += v;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
        for (int w = 0; w < SCAN_WAVES; w++) {
            const long long t = wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        __syncthreads();
        if (total <= a.dst_cap - carry) {
            // the round fits: every frame the source accepts is accepted
            if (f < a.nframes) {
                a.dst_off[f] = carry + before + inc - len;
                a.dst_frame_bytes[f] = (int32_t)len;
            }
            carry += total;
        } else {
            // a frame of this round does not fit; what follows it moves up by its length, so the round goes in order
            if (threadIdx.x == 0) {
                long long c = carry;
                const int end = base + SCAN_T < a.nframes ? base + SCAN_T : a.nframes;
                for (int g = base; g < end; g++) {
                    long long l = source_len(a, g);
                    if (l > a.dst_cap - c) l = 0;
                    a.dst_off[g] = c;
                    a.dst_frame_bytes[g] = (int32_t)l;
                    c += l;
                }
                wtot[0] = c;
            }
            __syncthreads();
            carry = wtot[0];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(COPY_T) void k_gather_frames(GatherFramesArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long f = (long long)blockIdx.x * COPY_FRAMES + (threadIdx.x >> 6);
    if (f >= a.nframes) return;
    const long long len = a.dst_frame_bytes[f], s = a.frame_src[f], o = a.dst_off[f];
    if (len < 1 || s < 0 || s > a.src_bytes - len || o < 0 || o > a.dst_cap - len) return;
    const uint8_t *src = a.src + s;
    uint8_t *dst = a.dst + o;
    long long head = (16 - (long long)(reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    if (head > len) head = len;
    const long long nq = (len - head) >> 4, tail = (len - head) & 15;
    if (lane < head) {
        dst[lane] = src[lane];
    } else if (lane >= 16 && lane - 16 < tail) {
        const long long i = head + (nq << 4) + (lane - 16);
        dst[i] = src[i];
    }
    const uint8_t *sb = src + head;
    uint4 *dq = reinterpret_cast<uint4 *>(dst + head);
    if ((reinterpret_cast<uintptr_t>(sb) & 15) == 0) {
        const uint4 *sq = reinterpret_cast<const uint4 *>(sb);
        for (long long q = lane; q < nq; q += 64) dq[q] = sq[q];
    } else {
        for (long long q = lane; q < nq; q += 64) {
            const uint8_t *p = sb + (q << 4);
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 |
                       (uint32_t)p[4 * k + 3] << 24;
            dq[q] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

}  // namespace

hipError_t launch_frame_heads(hipStream_t st, const FrameHeadsArgs &a)
{
    if (a.nframes < 1) return hipSuccess;
    note_launch("k_frame_heads");
    hipLaunchKernelGGL(k_frame_heads, dim3((unsigned)((a.nframes + HEADS_T - 1) / HEADS_T)), dim3(HEADS_T), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_frame_offsets(hipStream_t st, const FrameOffsetsArgs &a)
{
    if (a.nranges < 1 || a.frame_cap < 1) return hipSuccess;
    note_launch("k_frame_offsets");
    const int per = HEADS_T / 64;
    hipLaunchKernelGGL(k_frame_offsets, dim3((unsigned)((a.nranges + per - 1) / per)), dim3(HEADS_T), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_gather_offsets(hipStream_t st, const GatherFramesArgs &a)
{
    if (a.nframes < 1) return hipSuccess;
    note_launch("k_gather_offsets");
    hipLaunchKernelGGL(k_gather_offsets, dim3(1), dim3(SCAN_T), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_gather_frames(hipStream_t st, const GatherFramesArgs &a)
{
    if (a.nframes < 1) return hipSuccess;
    note_launch("k_gather_frames");
    hipLaunchKernelGGL(k_gather_frames, dim3((unsigned)((a.nframes + COPY_FRAMES - 1) / COPY_FRAMES)), dim3(COPY_T), 0, st, a);
    return hipGetLastError();
}

}  // namespace fhip
