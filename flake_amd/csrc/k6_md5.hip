// k6_md5.hip -- K6: the STREAMINFO MD5 (RFC 1321) of many streams at once.
//
// MD5 has no parallelism inside a stream -- the chain over 64-byte blocks and the 64 steps of a block are serial --
// and unlimited parallelism across streams: ONE LANE OWNS ONE STREAM.  A lane's work in a launch is a list of
// block_size-sample blocks of an interleaved PCM buffer (CSR: seg_first[nstreams + 1], seg_block[]), hashed in list
// order into the stream's fhip_md5_state.  The message bytes are what md5.c's fa_md5_pcm / fa_md5_pcm16 feed the
// hash: the low (bits_per_sample + 7) / 8 bytes of every interleaved sample, little-endian.
//
//   k_md5_init     the IVs
//   k_md5_scan     one workgroup: does any stream of the launch hold a partial block (fill != 0)?  -> flag
//   k_md5_streams  <sample type, bytes per sample>: the update.  Two paths, one launch-wide choice:
//       fast     the block's byte count is a multiple of 64 (the host knows) and no stream holds a partial block
//                (the flag): a block is a whole number of units (64 bytes; 192 at 3 bytes per sample), each built
//                in registers from 16-byte loads with constant indices, the next unit's loads issued before the
//                current unit's 64 steps;
//       general  any fill, any byte count: bytes go one by one through the lane's 64-byte tail in LDS (word-major:
//                word w of lane l at [w][l], no bank conflicts), hashed from there whenever it fills.
//   k_md5_final    padding + length into a copy of the state; 16 digest bytes per stream; the state stays usable.
//
// No path indexes registers dynamically; neither uses scratch (tests/test_md5_kernel_cpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"

namespace fhip {
namespace {

constexpr int MD5_WG = 64;          // one wave per workgroup: waves spread over the CUs, 4 KB of LDS each

#define MD5_F1(b, c, d) ((d) ^ ((b) & ((c) ^ (d))))
#define MD5_F2(b, c, d) ((c) ^ ((d) & ((b) ^ (c))))
#define MD5_F3(b, c, d) ((b) ^ (c) ^ (d))
#define MD5_F4(b, c, d) ((c) ^ ((b) | ~(d)))
#define MD5_STEP(f, a, b, c, d, w, k, s) \
    do { (a) += f((b), (c), (d)) + (w) + (k); (a) = __builtin_rotateleft32((a), (s)) + (b); } while (0)

// One 64-byte block, the 64 steps written out (RFC 1321 section 3.4); w[0..16) by constant index only.
__device__ __forceinline__ void md5_block(uint32_t (&h)[4], const uint32_t *__restrict__ w)
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    MD5_STEP(MD5_F1, a, b, c, d, w[0], 0xd76aa478u, 7);   MD5_STEP(MD5_F1, d, a, b, c, w[1], 0xe8c7b756u, 12);
    MD5_STEP(MD5_F1, c, d, a, b, w[2], 0x242070dbu, 17);  MD5_STEP(MD5_F1, b, c, d, a, w[3], 0xc1bdceeeu, 22);
    MD5_STEP(MD5_F1, a, b, c, d, w[4], 0xf57c0fafu, 7);   MD5_STEP(MD5_F1, d, a, b, c, w[5], 0x4787c62au, 12);
    MD5_STEP(MD5_F1, c, d, a, b, w[6], 0xa8304613u, 17);  MD5_STEP(MD5_F1, b, c, d, a, w[7], 0xfd469501u, 22);
    MD5_STEP(MD5_F1, a, b, c, d, w[8], 0x698098d8u, 7);   MD5_STEP(MD5_F1, d, a, b, c, w[9], 0x8b44f7afu, 12);
    MD5_STEP(MD5_F1, c, d, a, b, w[10], 0xffff5bb1u, 17); MD5_STEP(MD5_F1, b, c, d, a, w[11], 0x895cd7beu, 22);
    MD5_STEP(MD5_F1, a, b, c, d, w[12], 0x6b901122u, 7);  MD5_STEP(MD5_F1, d, a, b, c, w[13], 0xfd987193u, 12);
    MD5_STEP(MD5_F1, c, d, a, b, w[14], 0xa679438eu, 17); MD5_STEP(MD5_F1, b, c, d, a, w[15], 0x49b40821u, 22);

    MD5_STEP(MD5_F2, a, b, c, d, w[1], 0xf61e2562u, 5);   MD5_STEP(MD5_F2, d, a, b, c, w[6], 0xc040b340u, 9);
    MD5_STEP(MD5_F2, c, d, a, b, w[11], 0x265e5a51u, 14); MD5_STEP(MD5_F2, b, c, d, a, w[0], 0xe9b6c7aau, 20);
    MD5_STEP(MD5_F2, a, b, c, d, w[5], 0xd62f105du, 5);   MD5_STEP(MD5_F2, d, a, b, c, w[10], 0x02441453u, 9);
    MD5_STEP(MD5_F2, c, d, a, b, w[15], 0xd8a1e681u, 14); MD5_STEP(MD5_F2, b, c, d, a, w[4], 0xe7d3fbc8u, 20);
    MD5_STEP(MD5_F2, a, b, c, d, w[9], 0x21e1cde6u, 5);   MD5_STEP(MD5_F2, d, a, b, c, w[14], 0xc33707d6u, 9);
    MD5_STEP(MD5_F2, c, d, a, b, w[3], 0xf4d50d87u, 14);  MD5_STEP(MD5_F2, b, c, d, a, w[8], 0x455a14edu, 20);
    MD5_STEP(MD5_F2, a, b, c, d, w[13], 0xa9e3e905u, 5);  MD5_STEP(MD5_F2, d, a, b, c, w[2], 0xfcefa3f8u, 9);
    MD5_STEP(MD5_F2, c, d, a, b, w[7], 0x676f02d9u, 14);  MD5_STEP(MD5_F2, b, c, d, a, w[12], 0x8d2a4c8au, 20);

    MD5_STEP(MD5_F3, a, b, c, d, w[5], 0xfffa3942u, 4);   MD5_STEP(MD5_F3, d, a, b, c, w[8], 0x8771f681u, 11);
    MD5_STEP(MD5_F3, c, d, a, b, w[11], 0x6d9d6122u, 16); MD5_STEP(MD5_F3, b, c, d, a, w[14], 0xfde5380cu, 23);
    MD5_STEP(MD5_F3, a, b, c, d, w[1], 0xa4beea44u, 4);   MD5_STEP(MD5_F3, d, a, b, c, w[4], 0x4bdecfa9u, 11);
    MD5_STEP(MD5_F3, c, d, a, b, w[7], 0xf6bb4b60u, 16);  MD5_STEP(MD5_F3, b, c, d, a, w[10], 0xbebfbc70u, 23);
    MD5_STEP(MD5_F3, a, b, c, d, w[13], 0x289b7ec6u, 4);  MD5_STEP(MD5_F3, d, a, b, c, w[0], 0xeaa127fau, 11);
    MD5_STEP(MD5_F3, c, d, a, b, w[3], 0xd4ef3085u, 16);  MD5_STEP(MD5_F3, b, c, d, a, w[6], 0x04881d05u, 23);
    MD5_STEP(MD5_F3, a, b, c, d, w[9], 0xd9d4d039u, 4);   MD5_STEP(MD5_F3, d, a, b, c, w[12], 0xe6db99e5u, 11);
    MD5_STEP(MD5_F3, c, d, a, b, w[15], 0x1fa27cf8u, 16); MD5_STEP(MD5_F3, b, c, d, a, w[2], 0xc4ac5665u, 23);

    MD5_STEP(MD5_F4, a, b, c, d, w[0], 0xf4292244u, 6);   MD5_STEP(MD5_F4, d, a, b, c, w[7], 0x432aff97u, 10);
    MD5_STEP(MD5_F4, c, d, a, b, w[14], 0xab9423a7u, 15); MD5_STEP(MD5_F4, b, c, d, a, w[5], 0xfc93a039u, 21);
    MD5_STEP(MD5_F4, a, b, c, d, w[12], 0x655b59c3u, 6);  MD5_STEP(MD5_F4, d, a, b, c, w[3], 0x8f0ccc92u, 10);
    MD5_STEP(MD5_F4, c, d, a, b, w[10], 0xffeff47du, 15); MD5_STEP(MD5_F4, b, c, d, a, w[1], 0x85845dd1u, 21);
    MD5_STEP(MD5_F4, a, b, c, d, w[8], 0x6fa87e4fu, 6);   MD5_STEP(MD5_F4, d, a, b, c, w[15], 0xfe2ce6e0u, 10);
    MD5_STEP(MD5_F4, c, d, a, b, w[6], 0xa3014314u, 15);  MD5_STEP(MD5_F4, b, c, d, a, w[13], 0x4e0811a1u, 21);
    MD5_STEP(MD5_F4, a, b, c, d, w[4], 0xf7537e82u, 6);   MD5_STEP(MD5_F4, d, a, b, c, w[11], 0xbd3af235u, 10);
    MD5_STEP(MD5_F4, c, d, a, b, w[2], 0x2ad7d2bbu, 15);  MD5_STEP(MD5_F4, b, c, d, a, w[9], 0xeb86d391u, 21);
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
}

// A unit of the fast path: the fewest samples whose message bytes are whole 64-byte blocks.
template <class T, int BPS> struct Unit {
    static constexpr int SAMPLES = (BPS == 3) ? 64 : 64 / BPS;
    static constexpr int WORDS = SAMPLES * BPS / 4;              // 16, or 48 at 3 bytes per sample
    static constexpr int LOADS = SAMPLES * (int)sizeof(T) / 16;  // 16-byte loads
    static constexpr int RAW = LOADS * 4;                        // dwords they bring
};

// sample i (constant after unrolling) of a unit's raw dwords, as the low bits of a uint32 (sign bits above)
template <class T> __device__ __forceinline__ uint32_t unit_sample(const uint32_t *raw, int i)
{
    if constexpr (sizeof(T) == 4) return raw[i];
    else return (i & 1) ? (uint32_t)((int32_t)raw[i >> 1] >> 16) : (uint32_t)(int32_t)(int16_t)raw[i >> 1];
}

template <class T, int BPS>
__device__ __forceinline__ void unit_load(const T *__restrict__ p, uint32_t (&raw)[Unit<T, BPS>::RAW])
{
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < Unit<T, BPS>::LOADS; i++) {
        const uint4 v = q[i];
        raw[4 * i] = v.x; raw[4 * i + 1] = v.y; raw[4 * i + 2] = v.z; raw[4 * i + 3] = v.w;
    }
}

// raw samples -> the message dwords (little-endian: byte k of the message is bits 8(k & 3).. of word k / 4)
template <class T, int BPS>
__device__ __forceinline__ void unit_pack(const uint32_t (&raw)[Unit<T, BPS>::RAW], uint32_t (&w)[Unit<T, BPS>::WORDS])
{
    constexpr int W = Unit<T, BPS>::WORDS;
    if constexpr (BPS == 4) {
#pragma unroll
        for (int j = 0; j < W; j++) w[j] = raw[j];
    } else if constexpr (BPS == 2 && sizeof(T) == 2) {
#pragma unroll
        for (int j = 0; j < W; j++) w[j] = raw[j];                 // the buffer already is the image
    } else if constexpr (BPS == 2) {
#pragma unroll
        for (int j = 0; j < W; j++) w[j] = (raw[2 * j] & 0xFFFFu) | (raw[2 * j + 1] << 16);
    } else if constexpr (BPS == 1) {
#pragma unroll
        for (int j = 0; j < W; j++)
            w[j] = (unit_sample<T>(raw, 4 * j) & 0xFFu) | ((unit_sample<T>(raw, 4 * j + 1) & 0xFFu) << 8) |
                   ((unit_sample<T>(raw, 4 * j + 2) & 0xFFu) << 16) | (unit_sample<T>(raw, 4 * j + 3) << 24);
    } else {                                                       // 3 bytes: four samples -> three dwords
#pragma unroll
        for (int j = 0; j < W / 3; j++) {
            const uint32_t a = unit_sample<T>(raw, 4 * j) & 0xFFFFFFu, b = unit_sample<T>(raw, 4 * j + 1) & 0xFFFFFFu;
            const uint32_t c = unit_sample<T>(raw, 4 * j + 2) & 0xFFFFFFu, d = unit_sample<T>(raw, 4 * j + 3) & 0xFFFFFFu;
            w[3 * j] = a | (b << 24);
            w[3 * j + 1] = (b >> 8) | (c << 16);
            w[3 * j + 2] = (c >> 16) | (d << 8);
        }
    }
}

template <class T, int BPS>
__device__ __forceinline__ void unit_hash(uint32_t (&h)[4], const uint32_t (&raw)[Unit<T, BPS>::RAW])
{
    uint32_t w[Unit<T, BPS>::WORDS];
    unit_pack<T, BPS>(raw, w);
#pragma unroll
    for (int k = 0; k < Unit<T, BPS>::WORDS / 16; k++) md5_block(h, w + 16 * k);
}

// ---- general path: the lane's 64-byte tail in LDS, word w of lane l at tail[w * MD5_WG + l] ----
__device__ __forceinline__ void tail_hash(uint32_t (&h)[4], const uint32_t *tail, int lane)
{
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = tail[j * MD5_WG + lane];
    md5_block(h, w);
}

__device__ __forceinline__ void tail_put(uint32_t *tail, int lane, uint32_t fill, uint32_t byte)
{
    reinterpret_cast<uint8_t *>(tail + (fill >> 2) * MD5_WG + lane)[fill & 3u] = (uint8_t)byte;
}

__global__ void k_md5_init(fhip_md5_state *states, int nstreams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstreams) return;
    uint4 *q = reinterpret_cast<uint4 *>(states + s);
    q[0] = make_uint4(0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u);
#pragma unroll
    for (int i = 1; i < (int)(sizeof(fhip_md5_state) / 16); i++) q[i] = make_uint4(0, 0, 0, 0);
}

// flag[0] = 1 when any of the launch's streams holds a partial block; host_flag (pinned host memory, optional)
// receives the same, for fhip_last_launches.
__global__ void __launch_bounds__(1024) k_md5_scan(const fhip_md5_state *states, int nstreams, int32_t *flag,
                                                   int32_t *host_flag)
{
    __shared__ int any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    int mine = 0;
    for (int s = threadIdx.x; s < nstreams; s += blockDim.x) mine |= states[s].fill != 0;
    if (mine) any = 1;                       // (every writer stores the same value)
    __syncthreads();
    if (threadIdx.x == 0) {
        flag[0] = any;
        if (host_flag) host_flag[0] = any;
    }
}

template <class T, int BPS>
__global__ void __launch_bounds__(MD5_WG)
k_md5_streams(fhip_md5_state *__restrict__ states, int nstreams, const T *__restrict__ pcm, int block_vals,
              const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_block, int shape_fast,
              const int32_t *__restrict__ partial_flag)
{
    __shared__ uint32_t tail[16 * MD5_WG];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * MD5_WG + lane;
    if (s >= nstreams) return;
    const int b0 = seg_first[s], b1 = seg_first[s + 1];
    if (b1 <= b0) return;                    // no block in this launch: the state is not touched
    fhip_md5_state *st = states + s;
    uint32_t h[4];
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(st->h);
        h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
    }
    const uint64_t block_bytes = (uint64_t)block_vals * BPS;

    if (shape_fast && partial_flag[0] == 0) {                     // launch-wide, hence wave-uniform
        using U = Unit<T, BPS>;
        const int units = block_vals / U::SAMPLES;
        for (int b = b0; b < b1; b++) {
            const T *p = pcm + (size_t)seg_block[b] * (size_t)block_vals;
            uint32_t cur[U::RAW], nxt[U::RAW];
            unit_load<T, BPS>(p, cur);
            for (int u = 1; u < units; u++) {
                unit_load<T, BPS>(p + (size_t)u * U::SAMPLES, nxt);       // in flight during the 64 steps below
                unit_hash<T, BPS>(h, cur);
#pragma unroll
                for (int i = 0; i < U::RAW; i++) cur[i] = nxt[i];
            }
            unit_hash<T, BPS>(h, cur);
        }
        *reinterpret_cast<uint4 *>(st->h) = make_uint4(h[0], h[1], h[2], h[3]);
        st->nbytes += block_bytes * (uint64_t)(b1 - b0);
        return;
    }

    uint32_t fill = st->fill;
    {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) tail[j * MD5_WG + lane] = t[j];
    }
    for (int b = b0; b < b1; b++) {
        const T *p = pcm + (size_t)seg_block[b] * (size_t)block_vals;
        for (int i = 0; i < block_vals; i++) {
            uint32_t x = (uint32_t)(int32_t)p[i];
#pragma unroll
            for (int k = 0; k < BPS; k++) {
                tail_put(tail, lane, fill, x & 0xFFu);
                x >>= 8;
                if (++fill == 64) { tail_hash(h, tail, lane); fill = 0; }
            }
        }
    }
    *reinterpret_cast<uint4 *>(st->h) = make_uint4(h[0], h[1], h[2], h[3]);
    st->nbytes += block_bytes * (uint64_t)(b1 - b0);
    st->fill = fill;
    {
        uint32_t *t = reinterpret_cast<uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) t[j] = tail[j * MD5_WG + lane];
    }
}

// The general path for blocks of different lengths: block b of the tables is blk_vals[b] values at pcm + blk_off[b].
template <class T, int BPS>
__global__ void __launch_bounds__(MD5_WG)
k_md5_streams_ragged(fhip_md5_state *__restrict__ states, int nstreams, const T *__restrict__ pcm,
                     const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_block,
                     const long long *__restrict__ blk_off, const int32_t *__restrict__ blk_vals)
{
    __shared__ uint32_t tail[16 * MD5_WG];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * MD5_WG + lane;
    if (s >= nstreams) return;
    const int b0 = seg_first[s], b1 = seg_first[s + 1];
    if (b1 <= b0) return;                    // no block in this launch: the state is not touched
    fhip_md5_state *st = states + s;
    uint32_t h[4] = {st->h[0], st->h[1], st->h[2], st->h[3]};
    uint32_t fill = st->fill;
    {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) tail[j * MD5_WG + lane] = t[j];
    }
    uint64_t bytes = 0;
    for (int b = b0; b < b1; b++) {
        const int blk = seg_block[b];
        const T *p = pcm + (size_t)blk_off[blk];
        const int vals = blk_vals[blk];
        for (int i = 0; i < vals; i++) {
            uint32_t x = (uint32_t)(int32_t)p[i];
#pragma unroll
            for (int k = 0; k < BPS; k++) {
                tail_put(tail, lane, fill, x & 0xFFu);
                x >>= 8;
                if (++fill == 64) { tail_hash(h, tail, lane); fill = 0; }
            }
        }
        bytes += (uint64_t)vals * BPS;
    }
    st->h[0] = h[0]; st->h[1] = h[1]; st->h[2] = h[2]; st->h[3] = h[3];
    st->nbytes += bytes;
    st->fill = fill;
    {
        uint32_t *t = reinterpret_cast<uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) t[j] = tail[j * MD5_WG + lane];
    }
}

// A unit's raw dwords from an address that is only as aligned as T itself (a range starts at any sample, and the bytes
// taken to empty the tail move it further): the copies tell the compiler exactly that, and it picks loads that are
// legal there.  Nothing past the unit's last sample is read.
template <class T, int BPS>
__device__ __forceinline__ void unit_load_at_sample(const T *__restrict__ p, uint32_t (&raw)[Unit<T, BPS>::RAW])
{
#pragma unroll
    for (int i = 0; i < Unit<T, BPS>::LOADS; i++) {
        uint32_t v[4];
        __builtin_memcpy(v, p + i * (16 / (int)sizeof(T)), 16);
        raw[4 * i] = v[0]; raw[4 * i + 1] = v[1]; raw[4 * i + 2] = v[2]; raw[4 * i + 3] = v[3];
    }
}

// The update over ranges the device names: stream s absorbs, in order, the ranges seg_range[seg_first[s] ..
// seg_first[s + 1]); range r is the range_samples[r] samples per channel at sample range_start[r] of pcm (nch
// interleaved values each); a length <= 0 absorbs nothing.  Per range a lane (1) feeds samples through its tail until the
// tail is empty, (2) hashes whole units from registers, the next unit's loads in flight during the current one's steps,
// (3) feeds the rest through the tail.  The loops are plain structured loops, so the wave runs each phase together: in
// (2) every lane that still has a unit hashes one per trip and the others are masked off.  A tail that cannot empty on a
// sample boundary (a fill that is no multiple of the sample's bytes: never from whole samples at 1, 2 or 4 bytes) leaves
// everything to (1), which is correct at any fill.
template <class T, int BPS>
__global__ void __launch_bounds__(MD5_WG)
k_md5_ranges(fhip_md5_state *__restrict__ states, int nstreams, const T *__restrict__ pcm, int nch,
             const int32_t *__restrict__ seg_first, const int32_t *__restrict__ seg_range,
             const long long *__restrict__ range_start, const long long *__restrict__ range_samples)
{
    __shared__ uint32_t tail[16 * MD5_WG];
    using U = Unit<T, BPS>;
    const int lane = threadIdx.x;
    const int s = blockIdx.x * MD5_WG + lane;
    if (s >= nstreams) return;
    const int b0 = seg_first[s], b1 = seg_first[s + 1];
    if (b1 <= b0) return;                    // no range in this launch: the state is not touched
    fhip_md5_state *st = states + s;
    uint32_t h[4] = {st->h[0], st->h[1], st->h[2], st->h[3]};
    uint32_t fill = st->fill & 63u;
    {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) tail[j * MD5_WG + lane] = t[j];
    }
    uint64_t bytes = 0;
    for (int b = b0; b < b1; b++) {
        const int r = seg_range[b];
        const long long ns = range_samples[r];
        if (ns <= 0) continue;
        const long long vals = ns * nch;
        const T *p = pcm + (size_t)range_start[r] * (size_t)nch;
        bytes += (uint64_t)vals * BPS;
        long long i = 0;
        for (; i < vals && fill != 0; i++) {
            uint32_t x = (uint32_t)(int32_t)p[i];
#pragma unroll
            for (int k = 0; k < BPS; k++) {
                tail_put(tail, lane, fill, x & 0xFFu);
                x >>= 8;
                if (++fill == 64) { tail_hash(h, tail, lane); fill = 0; }
            }
        }
        const long long units = (vals - i) / U::SAMPLES;          // (fill is 0 here, or i == vals)
        if (units > 0) {
            const T *q = p + i;
            uint32_t cur[U::RAW], nxt[U::RAW];
            unit_load_at_sample<T, BPS>(q, cur);
            for (long long u = 1; u < units; u++) {
                unit_load_at_sample<T, BPS>(q + (size_t)u * U::SAMPLES, nxt);    // in flight during the 64 steps below
                unit_hash<T, BPS>(h, cur);
#pragma unroll
                for (int k = 0; k < U::RAW; k++) cur[k] = nxt[k];
            }
            unit_hash<T, BPS>(h, cur);
            i += units * U::SAMPLES;
        }
        for (; i < vals; i++) {
            uint32_t x = (uint32_t)(int32_t)p[i];
#pragma unroll
            for (int k = 0; k < BPS; k++) {
                tail_put(tail, lane, fill, x & 0xFFu);
                x >>= 8;
                if (++fill == 64) { tail_hash(h, tail, lane); fill = 0; }
            }
        }
    }
    st->h[0] = h[0]; st->h[1] = h[1]; st->h[2] = h[2]; st->h[3] = h[3];
    st->nbytes += bytes;
    st->fill = fill;
    {
        uint32_t *t = reinterpret_cast<uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) t[j] = tail[j * MD5_WG + lane];
    }
}

// fa_md5_final: 0x80, zeros up to 56 mod 64, the bit count; on a copy.
__global__ void __launch_bounds__(MD5_WG) k_md5_final(const fhip_md5_state *__restrict__ states, int nstreams,
                                                      uint8_t *__restrict__ digests)
{
    __shared__ uint32_t tail[16 * MD5_WG];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * MD5_WG + lane;
    if (s >= nstreams) return;
    const fhip_md5_state *st = states + s;
    uint32_t h[4] = {st->h[0], st->h[1], st->h[2], st->h[3]};
    const uint32_t fill = st->fill & 63u;
    const uint64_t bits = st->nbytes * 8u;
    {
        const uint32_t *t = reinterpret_cast<const uint32_t *>(st->tail);
#pragma unroll
        for (int j = 0; j < 16; j++) tail[j * MD5_WG + lane] = t[j];
    }
    tail_put(tail, lane, fill, 0x80u);
    for (uint32_t k = fill + 1; k < 64; k++) tail_put(tail, lane, k, 0);
    if (fill >= 56) {                        // no room for the length: it goes into a block of its own
        tail_hash(h, tail, lane);
#pragma unroll
        for (int j = 0; j < 14; j++) tail[j * MD5_WG + lane] = 0;
    }
    tail[14 * MD5_WG + lane] = (uint32_t)bits;
    tail[15 * MD5_WG + lane] = (uint32_t)(bits >> 32);
    tail_hash(h, tail, lane);
    uint32_t *d = reinterpret_cast<uint32_t *>(digests + (size_t)s * 16);
    d[0] = h[0]; d[1] = h[1]; d[2] = h[2]; d[3] = h[3];
}

template <class T, int BPS>
hipError_t launch_streams(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm, int block_vals,
                          const int32_t *seg_first, const int32_t *seg_block, bool shape_fast, const int32_t *flag)
{
    const int grid = (nstreams + MD5_WG - 1) / MD5_WG;
    hipLaunchKernelGGL((k_md5_streams<T, BPS>), dim3(grid), dim3(MD5_WG), 0, st, states, nstreams,
                       static_cast<const T *>(pcm), block_vals, seg_first, seg_block, shape_fast ? 1 : 0, flag);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_md5_init(hipStream_t st, fhip_md5_state *states, int nstreams)
{
    if (nstreams <= 0) return hipSuccess;
    note_launch("k_md5_init");
    hipLaunchKernelGGL(k_md5_init, dim3((nstreams + 255) / 256), dim3(256), 0, st, states, nstreams);
    return hipGetLastError();
}

bool md5_shape_fast(int block_vals, int bytes_per_sample, int pcm_format, const void *pcm)
{
    const size_t width = pcm_format == FHIP_PCM_S16 ? 2 : 4;
    // whole 64-byte blocks per PCM block (then also whole units: 192 bytes = 64 samples at 3 bytes each), and
    // every block of the buffer 16-byte aligned for the loads
    return ((size_t)block_vals * (size_t)bytes_per_sample) % 64 == 0 && ((uintptr_t)pcm & 15) == 0 &&
           ((size_t)block_vals * width) % 16 == 0;
}

hipError_t launch_md5_streams(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm, int pcm_format,
                              int block_vals, int bytes_per_sample, const int32_t *seg_first,
                              const int32_t *seg_block, int32_t *flag, int32_t *host_flag, bool *shape_fast_out)
{
    const bool s16 = pcm_format == FHIP_PCM_S16;
    const bool shape_fast = md5_shape_fast(block_vals, bytes_per_sample, pcm_format, pcm);
    if (shape_fast_out) *shape_fast_out = shape_fast;
    if (nstreams <= 0) return hipSuccess;
    if (shape_fast) {
        note_launch("k_md5_scan");
        hipLaunchKernelGGL(k_md5_scan, dim3(1), dim3(1024), 0, st, states, nstreams, flag, host_flag);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // (the path is appended to this entry once it is known: "fast" / "general", api.hip)
    note_launch("k_md5_streams<%s,%d>", s16 ? "int16_t" : "int32_t", bytes_per_sample);
    if (s16) {
        if (bytes_per_sample == 1) return launch_streams<int16_t, 1>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
        if (bytes_per_sample == 2) return launch_streams<int16_t, 2>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
        return hipErrorInvalidValue;
    }
    switch (bytes_per_sample) {
    case 1: return launch_streams<int32_t, 1>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
    case 2: return launch_streams<int32_t, 2>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
    case 3: return launch_streams<int32_t, 3>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
    case 4: return launch_streams<int32_t, 4>(st, states, nstreams, pcm, block_vals, seg_first, seg_block, shape_fast, flag);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_md5_streams_ragged(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm,
                                     int pcm_format, int bytes_per_sample, const int32_t *seg_first,
                                     const int32_t *seg_block, const long long *blk_off, const int32_t *blk_vals)
{
    if (nstreams <= 0) return hipSuccess;
    const bool s16 = pcm_format == FHIP_PCM_S16;
    if (bytes_per_sample < 1 || bytes_per_sample > (s16 ? 2 : 4)) return hipErrorInvalidValue;
    note_launch("k_md5_streams<%s,%d> ragged general", s16 ? "int16_t" : "int32_t", bytes_per_sample);
    const int grid = (nstreams + MD5_WG - 1) / MD5_WG;
#define LAUNCH_MR(T_, B_) hipLaunchKernelGGL((k_md5_streams_ragged<T_, B_>), dim3(grid), dim3(MD5_WG), 0, st, states, \
                                             nstreams, static_cast<const T_ *>(pcm), seg_first, seg_block, blk_off, blk_vals)
    if (s16) { if (bytes_per_sample == 1) LAUNCH_MR(int16_t, 1); else LAUNCH_MR(int16_t, 2); }
    else if (bytes_per_sample == 1) LAUNCH_MR(int32_t, 1);
    else if (bytes_per_sample == 2) LAUNCH_MR(int32_t, 2);
    else if (bytes_per_sample == 3) LAUNCH_MR(int32_t, 3);
    else LAUNCH_MR(int32_t, 4);
#undef LAUNCH_MR
    return hipGetLastError();
}

hipError_t launch_md5_ranges(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm, int pcm_format,
                             int bytes_per_sample, int channels, const int32_t *seg_first, const int32_t *seg_range,
                             const long long *range_start, const long long *range_samples)
{
    if (nstreams <= 0) return hipSuccess;
    const bool s16 = pcm_format == FHIP_PCM_S16;
    if (bytes_per_sample < 1 || bytes_per_sample > (s16 ? 2 : 4) || channels < 1) return hipErrorInvalidValue;
    note_launch("k_md5_ranges<%s,%d>", s16 ? "int16_t" : "int32_t", bytes_per_sample);
    const int grid = (nstreams + MD5_WG - 1) / MD5_WG;
#define LAUNCH_RG(T_, B_) hipLaunchKernelGGL((k_md5_ranges<T_, B_>), dim3(grid), dim3(MD5_WG), 0, st, states, nstreams, \
                                             static_cast<const T_ *>(pcm), channels, seg_first, seg_range, range_start, \
                                             range_samples)
    if (s16) { if (bytes_per_sample == 1) LAUNCH_RG(int16_t, 1); else LAUNCH_RG(int16_t, 2); }
    else if (bytes_per_sample == 1) LAUNCH_RG(int32_t, 1);
    else if (bytes_per_sample == 2) LAUNCH_RG(int32_t, 2);
    else if (bytes_per_sample == 3) LAUNCH_RG(int32_t, 3);
    else LAUNCH_RG(int32_t, 4);
#undef LAUNCH_RG
    return hipGetLastError();
}

hipError_t launch_md5_final(hipStream_t st, const fhip_md5_state *states, int nstreams, uint8_t *digests)
{
    if (nstreams <= 0) return hipSuccess;
    note_launch("k_md5_final");
    hipLaunchKernelGGL(k_md5_final, dim3((nstreams + MD5_WG - 1) / MD5_WG), dim3(MD5_WG), 0, st, states, nstreams,
                       digests);
    return hipGetLastError();
}

}  // namespace fhip
