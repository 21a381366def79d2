// k8_index.hip -- K8: frame discovery.  Where do the frames of a FLAC stream begin?  The answer is the CPU indexer's
// (flake_amd_index_frames, host/flake_decode.c), exactly, for every input, good or corrupt.
//
// A position is a CANDIDATE when a header that agrees with STREAMINFO and its own CRC-8 stands there: flac_header_ok
// (flac_header.h), the one function the CPU indexer compiles too.  A frame [a, q) is closed by a CRC-16 over
// [a, q - 2) that equals the two bytes at q - 2; this CRC has zero init and no final xor, so that is
// crc(s[a .. q)) == 0.  With
// P(p) = crc(s[0 .. p)) linearity gives P(q) = P(a) x^(8 (q - a)) + crc(s[a .. q)) in GF(2)[x] modulo the polynomial,
// and x is invertible there (the constant term is 1), so with key(p) = P(p) x^(-8 p) the condition is
// key(q) == key(a): two 16-bit values computed once per position.  The keys are an XOR prefix sum of the terms
// crc(chunk) x^(-8 end of chunk), so they need no multiplication to combine across lanes or workgroups.  x has order
// 32767 here (x^15 + x + 1 is primitive), so exponents are taken modulo that.
//
// Six launches, all on one stream:
//   k_index_scan<false>  a lane per IDX_LANE_BYTES of the stream: the lane's CRC term, the sync hits, the header
//                        predicate on every hit; per workgroup the candidate count and the XOR of the terms
//   k_index_wgscan       one workgroup: both exclusive scans over the workgroups, the candidate total
//   k_index_scan<true>   the same pass again; survivors go to the candidate table in position order with their keys
//   k_index_walk         a wave per range: the key at the range's end, then the walk from candidate 0.  Lane l asks
//                        whether candidate cur + l + 1 closes candidate cur + l -- almost always it does -- and the wave
//                        advances by the run of yeses (up to 63 frames a trip); where the neighbour does not close the
//                        frame the wave scans the later candidates, 64 a trip, then the range's end.  Only candidates
//                        the walk reaches are ever linked: a stream of false headers costs one scan, not one each.
//   k_index_ranges       one workgroup: where each range's sizes go (a scan of the counts), frame_cap, the
//                        per-range outputs
//   k_index_emit         a workgroup per range: the sizes
//
// Every stream read lies in [0, stream_bytes) and every read of the header predicate in the position's own range
// (clamped into the stream, whatever range_first holds); every table index is clamped to its array.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "flac_parse.h"            // CRC-16 and its GF(2) products, the workgroup scan

namespace fhip {
namespace {

constexpr int IDX_T = 256;                              // lanes of a scan workgroup
constexpr int IDX_LANE_BYTES = 16;                      // stream bytes per lane (one 16-byte load)
constexpr int IDX_WG_BYTES = IDX_T * IDX_LANE_BYTES;    // ... and per workgroup
constexpr int IDX_END_BYTES = 64;                       // k_index_walk: bytes per lane for the key at a range's end
constexpr uint32_t IDX_XINV8 = 0x7F81u;                 // x^(-8) modulo x^16 + x^15 + x^2 + 1
constexpr int IDX_XORDER = 32767;                       // the order of x

static_assert(IDX_END_BYTES * 64 == IDX_WG_BYTES, "a wave covers one scan workgroup's bytes");

static_assert(gf16_mul(IDX_XINV8, 0x100u) == 1u, "IDX_XINV8 is the inverse of x^8");

// r / x: the polynomial has constant term 1, so an odd r becomes even by adding it
constexpr uint32_t gf16_divx(uint32_t r) { return (r & 1u) ? ((r ^ 0x18005u) >> 1) : (r >> 1); }

// x^(-8 i) for i = 0 .. IDX_WG_BYTES: what moves a CRC taken at offset i of a workgroup's bytes to the key's frame
struct XinvTable {
    uint16_t v[IDX_WG_BYTES + 1];
    constexpr XinvTable() : v{}
    {
        uint32_t r = 1u;
        for (int i = 0; i <= IDX_WG_BYTES; i++) {
            v[i] = (uint16_t)r;
            for (int k = 0; k < 8; k++) r = gf16_divx(r);
        }
    }
};
constexpr XinvTable kXinvHost{};
static_assert(kXinvHost.v[1] == IDX_XINV8, "the table's step is x^(-8)");
__device__ const XinvTable c_xinv{};

// x^(-8 base) for a workgroup's first byte
__device__ uint32_t xinv_pow(long long base)
{
    const int e8 = (int)((base % IDX_XORDER) * 8 % IDX_XORDER);
    const int e = e8 ? IDX_XORDER - e8 : 0;             // x^(-k) = x^(order - k)
    uint32_t r = 1u;
    for (int bit = 14; bit >= 0; bit--) {
        r = gf16_mul(r, r);
        if ((e >> bit) & 1) r = (r & 0x8000u) ? (((r << 1) ^ 0x8005u) & 0xFFFFu) : (r << 1);
    }
    return r;
}

__device__ __forceinline__ long long clamp_off(long long v, long long bytes) { return v < 0 ? 0 : (v > bytes ? bytes : v); }

// range r of the call: [lo, hi) inside the stream, hi >= lo, whatever the table holds
__device__ __forceinline__ void range_bounds(const IndexArgs &a, int r, long long *lo, long long *hi)
{
    const long long l = clamp_off(a.range_first[r], a.stream_bytes), h = clamp_off(a.range_first[r + 1], a.stream_bytes);
    *lo = l;
    *hi = h < l ? l : h;
}

// the range position p lies in: the last r whose start is at or before p (ranges in front of it that share the start
// are empty).  false: p is in no range
__device__ bool range_of(const IndexArgs &a, long long p, long long *lo, long long *hi)
{
    int r = 0;
    if (a.nranges > 1) {
        int l = 0, h = a.nranges;                       // the answer is in [l, h)
        while (h - l > 1) {
            const int m = (l + h) >> 1;
            if (clamp_off(a.range_first[m], a.stream_bytes) <= p) l = m; else h = m;
        }
        r = l;
    }
    range_bounds(a, r, lo, hi);
    return p >= *lo && p < *hi;
}

// a candidate's packed fields: meta = len | vbs << 5 | n << 6, numkey = number (36 bits) | key << 48
__device__ __forceinline__ uint32_t pack_meta(const flac_header &h) { return (uint32_t)h.len | (uint32_t)h.vbs << 5 | (uint32_t)h.n << 6; }
__device__ __forceinline__ int meta_len(uint32_t m) { return (int)(m & 31u); }
__device__ __forceinline__ int meta_vbs(uint32_t m) { return (int)((m >> 5) & 1u); }
__device__ __forceinline__ int meta_n(uint32_t m) { return (int)(m >> 6); }
constexpr unsigned long long NUM_MASK = (1ull << 48) - 1ull;

// Exclusive scans over the workgroup, a sum and an XOR at once; *tc / *tx are the totals.
__device__ void block_scan2(int c, uint32_t x, int *sc, uint32_t *sx, int *ec, uint32_t *ex, int *tc, uint32_t *tx)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int ic = c;
    uint32_t ix = x;
    for (int d = 1; d < 64; d <<= 1) {
        const int oc = __shfl_up(ic, d, 64);
        const uint32_t ox = __shfl_up(ix, d, 64);
        if (lane >= d) { ic += oc; ix ^= ox; }
    }
    if (lane == 63) { sc[wid] = ic; sx[wid] = ix; }
    __syncthreads();
    int bc = 0, allc = 0;
    uint32_t bx = 0, allx = 0;
    for (int q = 0; q < IDX_T / 64; q++) {
        if (q < wid) { bc += sc[q]; bx ^= sx[q]; }
        allc += sc[q];
        allx ^= sx[q];
    }
    __syncthreads();
    *ec = bc + ic - c;
    *ex = bx ^ ix ^ x;
    *tc = allc;
    *tx = allx;
}

// The candidate pass.  SCATTER false: wg_cnt[g] = the workgroup's candidates, wg_key[g] = the XOR of its key terms.
// SCATTER true (behind k_index_wgscan, which turned both into exclusive prefixes): the table.
template <bool SCATTER>
__global__ void __launch_bounds__(IDX_T) k_index_scan(IndexArgs a)
{
    __shared__ int sc[IDX_T / 64];
    __shared__ uint32_t sx[IDX_T / 64];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * IDX_WG_BYTES, p0 = base + (long long)t * IDX_LANE_BYTES;
    long long left = a.stream_bytes - p0;
    const int cnt = left <= 0 ? 0 : (left > IDX_LANE_BYTES ? IDX_LANE_BYTES : (int)left);
    uint32_t w[IDX_LANE_BYTES / 4 + 1] = {0, 0, 0, 0, 0};       // the lane's bytes and the one behind them, little-endian
    if (cnt == IDX_LANE_BYTES && ((reinterpret_cast<uintptr_t>(a.stream) + (uintptr_t)p0) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.stream + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < IDX_LANE_BYTES; j++)
            if (j < cnt) w[j >> 2] |= (uint32_t)a.stream[p0 + j] << (8 * (j & 3));
    }
    if (left > IDX_LANE_BYTES) w[IDX_LANE_BYTES / 4] = a.stream[p0 + IDX_LANE_BYTES];
#define IDX_BYTE(j) ((w[(j) >> 2] >> (8 * ((j) & 3))) & 0xFFu)
    uint32_t crc = 0, syncs = 0;
#pragma unroll
    for (int j = 0; j < IDX_LANE_BYTES; j++) {
        if (j < cnt) {
            crc = crc16_byte(crc, IDX_BYTE(j));
            if (IDX_BYTE(j) == 0xFFu && (IDX_BYTE(j + 1) & 0xFEu) == 0xF8u) syncs |= 1u << j;
        }
    }
    const uint32_t term = cnt ? gf16_mul(crc, c_xinv.v[t * IDX_LANE_BYTES + cnt]) : 0u;
    // the header predicate on every sync hit (rare: bytes are read where they lie)
    int mine = 0;
    uint32_t good = 0;
    if (syncs) {
        for (int j = 0; j < IDX_LANE_BYTES; j++) {
            if (!((syncs >> j) & 1u)) continue;
            long long lo, hi;
            flac_header h;
            if (range_of(a, p0 + j, &lo, &hi) && flac_header_ok(&a.fmt, a.stream + p0 + j, hi - (p0 + j), &h)) {
                mine++;
                good |= 1u << j;
            }
        }
    }
    int ec, tc;
    uint32_t ex, tx;
    block_scan2(mine, term, sc, sx, &ec, &ex, &tc, &tx);
    const uint32_t wpow = xinv_pow(base);
    if (!SCATTER) {
        if (t == 0) {
            a.wg_cnt[blockIdx.x] = tc;
            a.wg_key[blockIdx.x] = gf16_mul(wpow, tx);
        }
        return;
    }
    if (!good) return;
    long long at = (long long)a.wg_cnt[blockIdx.x] + ec;
    const uint32_t key0 = a.wg_key[blockIdx.x];
    const uint64_t wl = w[0] | (uint64_t)w[1] << 32, wh = w[2] | (uint64_t)w[3] << 32;    // (no indexed registers below)
    uint32_t c = 0;
    for (int j = 0; j < IDX_LANE_BYTES; j++) {
        if ((good >> j) & 1u) {
            long long lo, hi;
            flac_header h;
            if (at < a.table_cap && range_of(a, p0 + j, &lo, &hi) && flac_header_ok(&a.fmt, a.stream + p0 + j, hi - (p0 + j), &h)) {
                const uint32_t key = key0 ^ gf16_mul(wpow, ex ^ gf16_mul(c, c_xinv.v[t * IDX_LANE_BYTES + j]));
                a.cand_pos[at] = (int32_t)(p0 + j);
                a.cand_meta[at] = pack_meta(h);
                a.cand_numkey[at] = (h.number & NUM_MASK) | (unsigned long long)key << 48;
            }
            at++;
        }
        c = crc16_byte(c, (uint32_t)((j < 8 ? wl : wh) >> (8 * (j & 7))) & 0xFFu);
    }
#undef IDX_BYTE
}

// One workgroup: wg_cnt and wg_key become exclusive prefixes ([nwg] of wg_key: the key at the stream's end),
// ncand[0] the candidate total.
__global__ void __launch_bounds__(IDX_T) k_index_wgscan(IndexArgs a)
{
    __shared__ int sc[IDX_T / 64];
    __shared__ uint32_t sx[IDX_T / 64];
    int carry_c = 0;
    uint32_t carry_x = 0;
    for (int g0 = 0; g0 < a.nwg; g0 += IDX_T) {
        const int g = g0 + threadIdx.x;
        const int c = g < a.nwg ? a.wg_cnt[g] : 0;
        const uint32_t x = g < a.nwg ? a.wg_key[g] : 0u;
        int ec, tc;
        uint32_t ex, tx;
        block_scan2(c, x, sc, sx, &ec, &ex, &tc, &tx);
        if (g < a.nwg) {
            a.wg_cnt[g] = carry_c + ec;
            a.wg_key[g] = carry_x ^ ex;
        }
        carry_c += tc;
        carry_x ^= tx;
    }
    if (threadIdx.x == 0) {
        a.wg_key[a.nwg] = carry_x;
        a.ncand[0] = carry_c;
    }
}

// the first table index whose position is at or behind p
__device__ int cand_lower_bound(const IndexArgs &a, int ncand, long long p)
{
    int l = 0, h = ncand;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (a.cand_pos[m] < p) l = m + 1; else h = m;
    }
    return l;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d, 64);
    return v;
}

// key(q) for a position that is no candidate (a range's end), by one wave: the prefix at q's workgroup, then the bytes
// from there to q, IDX_END_BYTES a lane
__device__ uint32_t key_at(const IndexArgs &a, long long q)
{
    const int lane = threadIdx.x & 63;
    const long long g = q / IDX_WG_BYTES, base = g * IDX_WG_BYTES;
    const int o = (int)(q - base);
    const uint32_t key0 = a.wg_key[g];                  // g <= nwg: q <= stream_bytes
    if (o == 0) return key0;
    int n = o - lane * IDX_END_BYTES;
    n = n < 0 ? 0 : (n > IDX_END_BYTES ? IDX_END_BYTES : n);
    uint32_t c = 0;
    const uint8_t *s = a.stream + base + lane * IDX_END_BYTES;
    for (int i = 0; i < n; i++) c = crc16_byte(c, s[i]);
    const uint32_t term = n ? gf16_mul(c, c_xinv.v[lane * IDX_END_BYTES + n]) : 0u;
    return key0 ^ gf16_mul(xinv_pow(base), wave_xor(term));
}

struct Cand { long long pos; uint32_t meta; unsigned long long numkey; };

// does the frame at candidate x end where candidate y begins?
__device__ __forceinline__ bool closes(const Cand &x, const Cand &y, int vbs)
{
    const unsigned long long want = (x.numkey & NUM_MASK) + (vbs ? (unsigned long long)meta_n(x.meta) : 1ull);
    return y.pos >= x.pos + meta_len(x.meta) + 2 && (y.numkey >> 48) == (x.numkey >> 48) && meta_vbs(y.meta) == vbs &&
           (y.numkey & NUM_MASK) == want;
}

// A wave per range.  Leaves rng_cf[r] (the range's first table index), rng_cnt[r] (frames found, before frame_cap; -1:
// the range does not begin with a header), rng_vbs[r], and in cand_end[rng_cf[r] + k] where frame k ends.
__global__ void __launch_bounds__(64) k_index_walk(IndexArgs a)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    long long lo, hi;
    range_bounds(a, r, &lo, &hi);
    long long nc = a.ncand[0];
    const int ncand = (int)(nc < a.table_cap ? nc : a.table_cap);
    const int cf = cand_lower_bound(a, ncand, lo), ce = cand_lower_bound(a, ncand, hi);
    int frames = 0, vbs = 0;
    if (hi > lo) {
        if (cf >= ce || a.cand_pos[cf] != lo) {
            frames = -1;
        } else {
            const uint32_t key_end = key_at(a, hi);
            vbs = meta_vbs(a.cand_meta[cf]);
            int cur = cf;
            for (;;) {
                // lane l: candidate cur + l and, from the lane above, its neighbour
                const int i = cur + lane;
                Cand x{0, 0, 0};
                if (i < ce) x = Cand{a.cand_pos[i], a.cand_meta[i], a.cand_numkey[i]};
                Cand y;
                y.pos = __shfl_down(x.pos, 1, 64);
                y.meta = __shfl_down(x.meta, 1, 64);
                y.numkey = __shfl_down(x.numkey, 1, 64);
                const bool ok = lane < 63 && i + 1 < ce && closes(x, y, vbs);
                const unsigned long long m = __ballot(ok);
                const int run = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
                if (run > 0) {
                    if (lane < run) a.cand_end[cf + frames + lane] = (int32_t)y.pos;
                    frames += run;
                    cur += run;
                    continue;
                }
                // the neighbour does not close the frame at cur: the first later candidate that does
                Cand x0;
                x0.pos = __shfl(x.pos, 0, 64);
                x0.meta = __shfl(x.meta, 0, 64);
                x0.numkey = __shfl(x.numkey, 0, 64);
                int found = -1;
                for (int j0 = cur + 1; j0 < ce && found < 0; j0 += 64) {
                    const int j = j0 + lane;
                    bool hit = false;
                    if (j < ce) hit = closes(x0, Cand{a.cand_pos[j], a.cand_meta[j], a.cand_numkey[j]}, vbs);
                    const unsigned long long mm = __ballot(hit);
                    if (mm) found = j0 + __ffsll((long long)mm) - 1;
                }
                if (found >= 0) {
                    if (lane == 0) a.cand_end[cf + frames] = a.cand_pos[found];
                    frames++;
                    cur = found;
                    continue;
                }
                // ... or the range's end
                if ((uint32_t)(x0.numkey >> 48) == key_end && hi >= x0.pos + meta_len(x0.meta) + 2) {
                    if (lane == 0) a.cand_end[cf + frames] = (int32_t)hi;
                    frames++;
                }
                break;
            }
        }
    }
    if (lane == 0) {
        a.rng_cf[r] = cf;
        a.rng_cnt[r] = frames;
        a.rng_vbs[r] = vbs;
    }
}

// One workgroup: range r's sizes go behind those of the ranges before it, as far as frame_cap allows; rng_off[r] and
// rng_cnt[r] (now the frames to write) tell k_index_emit.  Exactly the loop over flake_amd_index_frames with
// cap = frame_cap - frames so far: no room left gives 0 frames and 0 consumed before the header is looked at.
__global__ void __launch_bounds__(IDX_T) k_index_ranges(IndexArgs a)
{
    __shared__ long long ss[IDX_T / 64];
    long long carry = 0;
    for (int r0 = 0; r0 < a.nranges; r0 += IDX_T) {
        const int r = r0 + threadIdx.x;
        const int cnt = r < a.nranges ? a.rng_cnt[r] : 0;
        long long all = 0;
        const long long off = carry + block_excl_scan(cnt > 0 ? cnt : 0, ss, IDX_T / 64, &all);
        if (r < a.nranges) {
            const long long room = off < a.frame_cap ? a.frame_cap - off : 0;
            long long lo, hi;
            range_bounds(a, r, &lo, &hi);
            int frames = 0;
            long long consumed = 0;
            if (room > 0) {
                frames = cnt < 0 ? -1 : (cnt < room ? cnt : (int)room);
                if (frames > 0) consumed = a.cand_end[a.rng_cf[r] + frames - 1] - lo;
            }
            a.range_frames[r] = frames;
            a.range_consumed[r] = consumed;
            a.range_variable[r] = a.rng_vbs[r];
            a.rng_off[r] = off;
            a.rng_cnt[r] = frames > 0 ? frames : 0;
        }
        carry += all;
    }
}

__global__ void __launch_bounds__(IDX_T) k_index_emit(IndexArgs a)
{
    const int r = blockIdx.x;
    const int take = a.rng_cnt[r], cf = a.rng_cf[r];
    const long long off = a.rng_off[r];
    long long lo, hi;
    range_bounds(a, r, &lo, &hi);
    for (int k = threadIdx.x; k < take; k += IDX_T) {
        const long long prev = k ? a.cand_end[cf + k - 1] : lo;
        a.frame_bytes[off + k] = (int32_t)(a.cand_end[cf + k] - prev);
    }
}

const char *const kIndexStepNames[INDEX_STEPS] = {"k_index_scan<false>", "k_index_wgscan", "k_index_scan<true>",
                                                  "k_index_walk", "k_index_ranges", "k_index_emit"};

}  // namespace

const char *index_step_name(int step) { return step >= 0 && step < INDEX_STEPS ? kIndexStepNames[step] : ""; }

int index_nwg(long long stream_bytes) { return (int)((stream_bytes + IDX_WG_BYTES - 1) / IDX_WG_BYTES); }

void index_geometry(int *lane_bytes, int *wg_bytes, int *end_lane_bytes, int *xinv8)
{
    *lane_bytes = IDX_LANE_BYTES;
    *wg_bytes = IDX_WG_BYTES;
    *end_lane_bytes = IDX_END_BYTES;
    *xinv8 = (int)IDX_XINV8;
}

hipError_t launch_index_step(hipStream_t st, const IndexArgs &a, int step)
{
    switch (step) {
    case 0:
        if (a.nwg > 0) hipLaunchKernelGGL(k_index_scan<false>, dim3(a.nwg), dim3(IDX_T), 0, st, a);
        break;
    case 1: hipLaunchKernelGGL(k_index_wgscan, dim3(1), dim3(IDX_T), 0, st, a); break;
    case 2:
        if (a.nwg > 0) hipLaunchKernelGGL(k_index_scan<true>, dim3(a.nwg), dim3(IDX_T), 0, st, a);
        break;
    case 3: hipLaunchKernelGGL(k_index_walk, dim3(a.nranges), dim3(64), 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_index_ranges, dim3(1), dim3(IDX_T), 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_index_emit, dim3(a.nranges), dim3(IDX_T), 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    if (step == 1 || step >= 3 || a.nwg > 0) note_launch("%s", kIndexStepNames[step]);
    return hipGetLastError();
}

}  // namespace fhip
