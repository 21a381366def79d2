// k10_rows.hip -- K10: what K7's window mode left back to back and channel-interleaved in one device buffer, re-laid as a
// padded planar batch rows[nrows][channels][row_len] in another: int32 as it is, int16, or float32 scaled to [-1, 1).
// What lets a caller on the same device -- a training loop that crops a corpus -- take windows where they were decoded.
//
// A segment k is seg_samples[k] samples per channel at sample seg_start[k] of pcm (K7's outputs, read where K7 left
// them) and goes to row seg_row[k] from column seg_col[k] on (the caller's tables).  It is delivered when
// seg_failed[k] < 0, 0 <= seg_row[k] < nrows, 0 <= seg_col[k] < row_len and 0 <= seg_start[k] < pcm_cap, and then
// delivers min(seg_samples[k], row_len - seg_col[k], pcm_cap - seg_start[k]) samples (none where that is not positive).
// Nothing else is written: the kernel zeroes nothing.
//
// Segments run from one sample to a whole row, so the work is dealt out by segment AND tile of ROWS_TILE samples: the
// grid holds, for every segment, the tiles of the longest segment there can be (min(row_len, pcm_cap) samples), and a
// workgroup whose tile lies behind its segment's end leaves after five table reads.  A tile goes through LDS:
//   in   the tile's samples * channels interleaved values are one contiguous span of pcm; lanes take it in groups of
//        four values that start on 16-byte boundaries OF THE SOURCE (the grouping is shifted by the span's
//        misalignment), so every group inside the span is one 16-byte load whatever seg_start and the channel count
//        are; the span's first and last partial group load value by value.  Each value lands in its channel's line of
//        the tile in LDS.
//   out  a lane takes four consecutive samples of one channel from LDS, converts them and stores them with one
//        16-byte store (8 bytes for int16) where the destination address allows, value by value elsewhere (an odd
//        row_len, a column that is no multiple of four, the tile's end): consecutive lanes, consecutive addresses.
// One body for every channel count 1 .. 8 and every row_len; the format is a template argument.
//
// Memory safety is structural, as K7's, K8's and K9's: every table index is clamped to [0, nsegs), every read into
// [0, pcm_cap * channels), every write lies in the row's own [0, row_len) of a row inside [0, nrows) -- whatever the
// device tables hold.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "rows_tile.h"

namespace fhip {
namespace {

template <int FMT> __global__ __launch_bounds__(ROWS_T) void k_window_rows(WindowRowsArgs a)
{
    using E = typename RowsElem<FMT>::type;
    __shared__ __attribute__((aligned(16))) int32_t tile[ROWS_MAX_CH * ROWS_TILE];

    const int ch = a.channels < 1 ? 1 : (a.channels > ROWS_MAX_CH ? ROWS_MAX_CH : a.channels);
    // wave-uniform: the segment and the tile of this workgroup
    if (a.nsegs < 1 || a.tiles < 1 || a.pcm_cap < 1 || a.row_len < 1) return;
    const unsigned kk = blockIdx.x / (unsigned)a.tiles;
    const long long t0 = (long long)(blockIdx.x - kk * (unsigned)a.tiles) * ROWS_TILE;    // the tile's first sample in the segment
    const int k = kk < (unsigned)a.nsegs ? (int)kk : a.nsegs - 1;
    const int row = a.seg_row[k];
    const long long col = a.seg_col[k], start = a.seg_start[k];
    long long n = a.seg_samples[k];
    if (a.seg_failed[k] >= 0 || row < 0 || row >= a.nrows || col < 0 || col >= a.row_len || start < 0 || start >= a.pcm_cap)
        return;
    if (n > a.row_len - col) n = a.row_len - col;
    if (n > a.pcm_cap - start) n = a.pcm_cap - start;
    if (t0 >= n) return;                                                  // (n <= 0 included: the surplus leaves here)
    const int nt = n - t0 < ROWS_TILE ? (int)(n - t0) : ROWS_TILE;        // samples of this tile, 1 .. ROWS_TILE
    const int nvals = nt * ch;

    // in: the span of pcm that holds the tile, into LDS
    rows_tile_load(tile, a.pcm, a.pcm_cap * ch, (start + t0) * ch, nvals, ch);
    __syncthreads();

    // out: four consecutive samples of one channel per lane
    constexpr int QUADS = ROWS_TILE / 4;
    E *const rows = static_cast<E *>(a.rows);
    for (int it = threadIdx.x; it < ch * QUADS; it += ROWS_T) {
        const int c = it / QUADS, i0 = 4 * (it - c * QUADS);
        if (i0 >= nt) continue;
        const int4 q = *reinterpret_cast<const int4 *>(&tile[c * ROWS_TILE + i0]);
        const E e[4] = {rows_conv<FMT>(q.x, a.scale), rows_conv<FMT>(q.y, a.scale), rows_conv<FMT>(q.z, a.scale),
                        rows_conv<FMT>(q.w, a.scale)};
        E *const dst = rows + ((long long)row * ch + c) * a.row_len + col + t0 + i0;     // col + t0 + i0 < col + n <= row_len
        if (i0 + 4 <= nt && (reinterpret_cast<uintptr_t>(dst) & (4 * sizeof(E) - 1)) == 0) {
            struct alignas(4 * sizeof(E)) Quad { E x[4]; };
            *reinterpret_cast<Quad *>(dst) = Quad{{e[0], e[1], e[2], e[3]}};
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (i0 + j < nt) dst[j] = e[j];
        }
    }
}

}  // namespace

hipError_t launch_window_rows(hipStream_t st, const WindowRowsArgs &args)
{
    WindowRowsArgs a = args;
    if (a.nsegs < 1 || a.pcm_cap < 1 || a.row_len < 1 || a.nrows < 1) return hipSuccess;
    if (a.channels < 1 || a.channels > ROWS_MAX_CH) return hipErrorInvalidValue;
    // the longest segment there can be: a row's length, and no more than the source holds
    const long long longest = a.row_len < a.pcm_cap ? a.row_len : a.pcm_cap;
    const long long tiles = (longest + ROWS_TILE - 1) / ROWS_TILE, wgs = tiles * a.nsegs;
    if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
    if (a.format != FHIP_ROWS_I32 && a.format != FHIP_ROWS_I16 && a.format != FHIP_ROWS_F32) return hipErrorInvalidValue;
    a.tiles = (int)tiles;
    note_launch("k_window_rows");
    const dim3 grid((unsigned)wgs), block(ROWS_T);
    switch (a.format) {
    case FHIP_ROWS_I32: hipLaunchKernelGGL(k_window_rows<FHIP_ROWS_I32>, grid, block, 0, st, a); break;
    case FHIP_ROWS_I16: hipLaunchKernelGGL(k_window_rows<FHIP_ROWS_I16>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(k_window_rows<FHIP_ROWS_F32>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

}  // namespace fhip
