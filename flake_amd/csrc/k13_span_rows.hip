// k13_span_rows.hip -- K13: K10's re-layout, one to many.  What K7's window mode left back to back and channel-interleaved
// is a SPAN of a stream here -- a long run decoded once -- and rows[nrows][channels][row_len] takes every window of
// row_len samples that begins hop samples behind the one before it: int32 as it is, int16, or float32 scaled to [-1, 1).
// What lets a caller on the same device walk whole recordings in overlapping chunks with every frame decoded once.
//
// A segment k is seg_samples[k] samples per channel at sample seg_start[k] of pcm (K7's outputs, read where K7 left
// them); its first sample is sample seg_pos[k] of its span, and the span owns the seg_nrows[k] rows from seg_row0[k] on
// (the caller's tables).  It is delivered when seg_failed[k] < 0, seg_nrows[k] >= 1, seg_row0[k] >= 0,
// seg_row0[k] + seg_nrows[k] <= nrows, seg_pos[k] >= 0 and 0 <= seg_start[k] < pcm_cap.  Sample
// i < min(seg_samples[k], pcm_cap - seg_start[k]) is at span position p = seg_pos[k] + i and is written to column
// p - j * hop of row seg_row0[k] + j for every j in [0, seg_nrows[k]) with j * hop <= p < j * hop + row_len.  Nothing
// else is written: the kernel zeroes nothing.
//
// Segments run from one sample to a whole stream, so the launch is not sized by the longest: the caller allots every
// segment its tiles of ROWS_TILE samples in a CSR (tile_first), from an upper bound of the segment's length it has
// before K7 has run, and a workgroup finds its segment there by bisection.  A tile behind its segment's end leaves
// after the table reads; samples behind a segment's allotted tiles are not delivered.  A tile goes through LDS:
//   in   exactly K10's: the tile's samples * channels interleaved values are one contiguous span of pcm, taken in
//        groups of four values on 16-byte boundaries OF THE SOURCE, each value into its channel's line of the tile.
//   out  the tile overlaps the rows j with j * hop < P + nt and j * hop + row_len > P (P its first span position), and
//        the work is (row, channel, quad) with the quad running fastest: consecutive lanes, consecutive addresses.
//        The quads lie on 16-byte boundaries OF THE DESTINATION (8 bytes for int16), so that every quad inside a row's
//        share of the tile is one wide store whatever hop, row_len and the column are; the row's first and last partial
//        quad store value by value.  A quad's four values lie anywhere in the channel's line: a lane takes the two
//        aligned 16-byte groups around them from LDS and picks.
// One body for every channel count 1 .. 8, every row_len and every hop; the format is a template argument.
//
// Memory safety is structural, as K10's: every table index is clamped to [0, nsegs), every read into
// [0, pcm_cap * channels), every write lies in the row's own [0, row_len) of a row inside
// [seg_row0, seg_row0 + seg_nrows), itself inside [0, nrows) -- whatever the device tables hold.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "rows_tile.h"

namespace fhip {
namespace {

constexpr int SPAN_ROWS_PASS = 1 << 16;                         // rows per pass of the out loop: its index stays an int

template <int FMT> __global__ __launch_bounds__(ROWS_T) void k_span_rows(SpanRowsArgs a)
{
    using E = typename RowsElem<FMT>::type;
    __shared__ __attribute__((aligned(16))) int32_t tile[ROWS_MAX_CH * ROWS_TILE];

    const int ch = a.channels < 1 ? 1 : (a.channels > ROWS_MAX_CH ? ROWS_MAX_CH : a.channels);
    // wave-uniform: the segment and the tile of this workgroup
    if (a.nsegs < 1 || a.pcm_cap < 1 || a.row_len < 1 || a.hop < 1 || a.nrows < 1) return;
    const long long wg = blockIdx.x;
    int k = 0;
    for (int hi = a.nsegs - 1; k < hi;) {                                 // the last segment whose first tile is not behind wg
        const int mid = k + (hi - k + 1) / 2;
        if (a.tile_first[mid] <= wg) k = mid; else hi = mid - 1;
    }
    const long long t = wg - a.tile_first[k];
    if (t < 0 || t > 0x7FFFFFFFll / ROWS_TILE) return;
    const long long t0 = t * ROWS_TILE;                                   // the tile's first sample in the segment
    const long long row0 = a.seg_row0[k], nr = a.seg_nrows[k];
    const long long pos = a.seg_pos[k], start = a.seg_start[k];
    long long n = a.seg_samples[k];
    if (a.seg_failed[k] >= 0 || nr < 1 || row0 < 0 || row0 + nr > a.nrows || pos < 0 || pos > (1ll << 62) || start < 0 ||
        start >= a.pcm_cap)
        return;
    if (n > a.pcm_cap - start) n = a.pcm_cap - start;
    if (t0 >= n) return;                                                  // (n <= 0 included: the surplus leaves here)
    const int nt = n - t0 < ROWS_TILE ? (int)(n - t0) : ROWS_TILE;        // samples of this tile, 1 .. ROWS_TILE
    const int nvals = nt * ch;
    // the rows the tile overlaps: j * hop <= P + nt - 1 and j * hop + row_len > P  (nr <= 2^31, hop < 2^31: no overflow)
    const long long P = pos + t0;
    long long jhi = (P + nt - 1) / a.hop;
    if (jhi > nr - 1) jhi = nr - 1;
    const long long jlo = P >= a.row_len ? (P - a.row_len) / a.hop + 1 : 0;
    if (jlo > jhi) return;                                                // (the tile lies between two rows: hop > row_len)

    // in: the span of pcm that holds the tile, into LDS
    rows_tile_load(tile, a.pcm, a.pcm_cap * ch, (start + t0) * ch, nvals, ch);
    __syncthreads();

    // out: a row's share of the tile is at most L samples, which no more than QPR destination quads cover
    const int L = a.row_len < nt ? (int)a.row_len : nt;
    const int QPR = (L + 6) >> 2, per = ch * QPR;                         // per <= 8 * 129
    E *const rows = static_cast<E *>(a.rows);
    for (long long jb = jlo; jb <= jhi; jb += SPAN_ROWS_PASS) {
        const int jn = jhi - jb + 1 < SPAN_ROWS_PASS ? (int)(jhi - jb + 1) : SPAN_ROWS_PASS;
        for (int it = threadIdx.x; it < jn * per; it += ROWS_T) {
            const int dj = it / per, r = it - dj * per, c = r / QPR, q = r - c * QPR;
            const long long j = jb + dj, r0 = j * a.hop;                  // the row's first span position
            const long long lo = r0 > P ? r0 : P;                         // the row's share of the tile: [lo, lo + len)
            const long long room = a.row_len - (lo - r0);                 // (>= 1: j >= jlo)
            const int il = (int)(lo - P);                                 // (< nt: j <= jhi)
            const int len = room < nt - il ? (int)room : nt - il;
            E *const dst = rows + ((row0 + j) * ch + c) * a.row_len + (lo - r0);       // the share's first element
            const int dmis = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(E)) & 3);
            const int f = 4 * q - dmis;                                   // the quad's first value in the share
            if (f >= len) continue;
            // the values tile[i .. i + 4) of the channel's line, i = il + f in [-3, nt): two aligned groups around them
            const int i = il + f, al = i & ~3, s = i & 3;
            const int a0 = al < 0 ? 0 : al, a1 = al + 4 > ROWS_TILE - 4 ? ROWS_TILE - 4 : al + 4;
            const int4 g0 = *reinterpret_cast<const int4 *>(&tile[c * ROWS_TILE + a0]);
            const int4 g1 = *reinterpret_cast<const int4 *>(&tile[c * ROWS_TILE + a1]);
            const int32_t v[7] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z};
            E e[4];
#pragma unroll
            for (int m = 0; m < 4; m++)
                e[m] = rows_conv<FMT>(s == 0 ? v[m] : (s == 1 ? v[m + 1] : (s == 2 ? v[m + 2] : v[m + 3])), a.scale);
            if (f >= 0 && f + 4 <= len && (reinterpret_cast<uintptr_t>(dst + f) & (4 * sizeof(E) - 1)) == 0) {
                struct alignas(4 * sizeof(E)) Quad { E x[4]; };
                *reinterpret_cast<Quad *>(dst + f) = Quad{{e[0], e[1], e[2], e[3]}};
            } else {
#pragma unroll
                for (int m = 0; m < 4; m++)
                    if (f + m >= 0 && f + m < len) dst[f + m] = e[m];     // (lo - r0 + f + m < lo - r0 + len <= row_len)
            }
        }
    }
}

}  // namespace

hipError_t launch_span_rows(hipStream_t st, const SpanRowsArgs &a)
{
    if (a.nsegs < 1 || a.ntiles < 1 || a.pcm_cap < 1 || a.row_len < 1 || a.nrows < 1) return hipSuccess;
    if (a.channels < 1 || a.channels > ROWS_MAX_CH || a.hop < 1 || a.hop > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (a.format != FHIP_ROWS_I32 && a.format != FHIP_ROWS_I16 && a.format != FHIP_ROWS_F32) return hipErrorInvalidValue;
    note_launch("k_span_rows");
    const dim3 grid((unsigned)a.ntiles), block(ROWS_T);
    switch (a.format) {
    case FHIP_ROWS_I32: hipLaunchKernelGGL(k_span_rows<FHIP_ROWS_I32>, grid, block, 0, st, a); break;
    case FHIP_ROWS_I16: hipLaunchKernelGGL(k_span_rows<FHIP_ROWS_I16>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(k_span_rows<FHIP_ROWS_F32>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace fhip
