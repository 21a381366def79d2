// k12_rows_in.hip -- K12: the inverse of K10.  Spans of a padded planar batch rows[nrows][channels][row_len] in device
// memory -- int32, int16 or float32 -- converted and laid channel-interleaved as int32 into one destination: what lets
// audio that already is a tensor on the device (a model's output, a corpus that was resampled there) be encoded without
// the samples crossing the link.  The destination is a handle's PCM staging, or any buffer of the caller's.
//
// A piece is {row, count, col, dst} in samples per channel: count samples from column col of row `row` go to sample dst
// of the destination.  The pieces are sorted by dst and tile [0, total) (the host entry has checked that; the kernel does
// not rely on it).  Pieces run from one sample to a whole row, so the work is dealt out by DESTINATION, as K9's is: a
// workgroup owns one tile of ROWS_IN_TILE samples, a lane four consecutive samples of every channel.  The tile's first
// and last piece are found by two wave-uniform binary searches; a lane then searches only between those two.
//
// A lane whose four samples lie in one piece reads, for each channel, the four consecutive columns with one 16-byte load
// (8 bytes for int16) where that address is so aligned, element by element elsewhere (an odd row_len puts the channel
// planes at different offsets modulo 16, so the choice is made per channel); a lane with a piece boundary inside its
// four samples reads element by element.  It converts, and writes its 4 * channels interleaved values -- one contiguous
// span -- with 16-byte stores where the destination is 16-byte aligned and all four samples are written.
//
// Conversion of element e to sample x, b = bits_per_sample:
//   int32    x = e
//   int16    x = e, sign-extended
//   float32  x = clamp(rne(e * 2^(b-1)), -2^(b-1), 2^(b-1) - 1), NaN -> 0: the product is exact (a power of two), rne is
//            round to nearest, ties to even, and the clamp is made on the float side, where 2^(b-1) is exact, before the
//            conversion to int.  The inverse of K10's float32 for every sample of up to 24 bits.
//
// Memory safety is structural, as K9's: every table index is clamped to [0, npieces), every read lies inside
// nrows * channels * row_len elements (row and column are clamped separately), every write lies below both the table's
// total and the destination's capacity -- whatever the device table holds.  No LDS, no scratch: the channel count is a
// template argument, so a lane's values are registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "rows_tile.h"

namespace fhip {
namespace {

constexpr int ROWS_IN_T = 256;                                  // lanes of a workgroup
constexpr int ROWS_IN_LANE = 4;                                 // destination samples of a lane
static_assert(ROWS_IN_T * ROWS_IN_LANE == ROWS_IN_TILE, "a workgroup covers one tile");

// two_pow = 2^(b-1) as a float (exact for every b <= 32); imax = 2^(b-1) - 1
template <int FMT> __device__ inline int32_t rows_in_conv(typename RowsElem<FMT>::type e, float two_pow, int32_t imax)
{
    if constexpr (FMT == FHIP_ROWS_F32) {
        const float r = rintf(e * two_pow);                     // exact product, then round to nearest even
        if (!(r == r)) return 0;                                // NaN
        if (r >= two_pow) return imax;                          // (+inf included; at b = 32 everything from 2^31 on)
        if (r <= -two_pow) return -imax - 1;
        return (int32_t)r;                                      // |r| < 2^(b-1) <= 2^31: in range
    } else {
        return (int32_t)e;
    }
}

// (eight waves per SIMD: a lane's 4 * CH values and its addresses fit 64 registers for every CH, and nothing but
// occupancy hides the latency of a conversion that is all loads and stores)
template <int FMT, int CH> __global__ __launch_bounds__(ROWS_IN_T) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_rows_to_pcm(RowsInArgs a)
{
    using E = typename RowsElem<FMT>::type;
    struct alignas(4 * sizeof(E)) Quad { E x[4]; };
    // what may be written: below the table's total and the destination's capacity (samples per channel)
    const long long lim_s = a.total < a.dst_cap ? a.total : a.dst_cap;
    const long long lim = lim_s > 0 ? lim_s : 0;
    const long long tile0 = (long long)blockIdx.x * ROWS_IN_TILE;
    if (tile0 >= lim || a.npieces < 1 || a.nrows < 1 || a.row_len < 1) return;
    const long long tile_last = (tile0 + ROWS_IN_TILE < lim ? tile0 + ROWS_IN_TILE : lim) - 1;
    // wave-uniform: the pieces of the tile's first and last sample
    const int last = a.npieces - 1;
    const int p_lo = piece_at(a.pieces, 0, last, tile0);
    const int p_hi = piece_at(a.pieces, p_lo, last, tile_last);

    const long long s0 = tile0 + (long long)threadIdx.x * ROWS_IN_LANE;
    if (s0 >= lim) return;
    int pi = p_lo == p_hi ? p_lo : piece_at(a.pieces, p_lo, p_hi, s0);
    RowPiece p = a.pieces[pi];
    long long end = p.dst + p.count;                            // the piece's end in the destination
    const E *const rows = static_cast<const E *>(a.rows);
    const bool whole = s0 + ROWS_IN_LANE <= lim;

    int32_t v[ROWS_IN_LANE][CH];
#pragma unroll
    for (int k = 0; k < ROWS_IN_LANE; k++)
#pragma unroll
        for (int c = 0; c < CH; c++) v[k][c] = 0;

    const long long col0 = p.col + (s0 - p.dst);
    if (whole && s0 + ROWS_IN_LANE <= end && p.row >= 0 && p.row < a.nrows && col0 >= 0 && col0 + ROWS_IN_LANE <= a.row_len) {
        // one piece: four consecutive columns of every channel
        const E *src = rows + (long long)p.row * CH * a.row_len + col0;
#pragma unroll
        for (int c = 0; c < CH; c++, src += a.row_len) {
            E e[4];
            if ((reinterpret_cast<uintptr_t>(src) & (4 * sizeof(E) - 1)) == 0) {
                const Quad q = *reinterpret_cast<const Quad *>(src);
                e[0] = q.x[0]; e[1] = q.x[1]; e[2] = q.x[2]; e[3] = q.x[3];
            } else {
                e[0] = src[0]; e[1] = src[1]; e[2] = src[2]; e[3] = src[3];
            }
#pragma unroll
            for (int k = 0; k < ROWS_IN_LANE; k++) v[k][c] = rows_in_conv<FMT>(e[k], a.two_pow, a.imax);
        }
    } else {
#pragma unroll
        for (int k = 0; k < ROWS_IN_LANE; k++) {
            const long long at = s0 + k;
            if (at >= lim) break;
            // on to the piece that holds this sample: pieces are at least one sample long in a table the host took,
            // and the walk ends at the tile's last piece whatever the table holds
            while (at >= end && pi < p_hi) {
                p = a.pieces[++pi];
                end = p.dst + p.count;
            }
            long long row = p.row, col = p.col + (at - p.dst);
            row = row < 0 ? 0 : (row >= a.nrows ? a.nrows - 1 : row);
            col = col < 0 ? 0 : (col >= a.row_len ? a.row_len - 1 : col);
            const E *src = rows + row * CH * a.row_len + col;
#pragma unroll
            for (int c = 0; c < CH; c++, src += a.row_len) v[k][c] = rows_in_conv<FMT>(*src, a.two_pow, a.imax);
        }
    }

    // the lane's 4 * CH interleaved values are one contiguous span of the destination
    int32_t *const dst = a.dst + s0 * CH;
    if (whole && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < CH; j++) {                          // value 4 j + i is sample (4 j + i) / CH, channel (4 j + i) % CH
            reinterpret_cast<int4 *>(dst)[j] = make_int4(v[(4 * j) / CH][(4 * j) % CH], v[(4 * j + 1) / CH][(4 * j + 1) % CH],
                                                         v[(4 * j + 2) / CH][(4 * j + 2) % CH], v[(4 * j + 3) / CH][(4 * j + 3) % CH]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < ROWS_IN_LANE; k++) {
            if (s0 + k >= lim) break;
#pragma unroll
            for (int c = 0; c < CH; c++) dst[k * CH + c] = v[k][c];
        }
    }
}

template <int FMT> hipError_t launch_fmt(hipStream_t st, const RowsInArgs &a, dim3 grid)
{
    const dim3 block(ROWS_IN_T);
    switch (a.channels) {
    case 1: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 3>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 4>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 5>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 6>), grid, block, 0, st, a); break;
    case 7: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 7>), grid, block, 0, st, a); break;
    case 8: hipLaunchKernelGGL((k_rows_to_pcm<FMT, 8>), grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rows_to_pcm(hipStream_t st, const RowsInArgs &args)
{
    RowsInArgs a = args;
    if (a.npieces < 1 || a.total < 1 || a.dst_cap < 1) return hipSuccess;
    if (a.nrows < 1 || a.row_len < 1 || a.channels < 1 || a.channels > 8 || a.bits < 1 || a.bits > 32) return hipErrorInvalidValue;
    if (a.format != FHIP_ROWS_I32 && a.format != FHIP_ROWS_I16 && a.format != FHIP_ROWS_F32) return hipErrorInvalidValue;
    const long long lim = a.total < a.dst_cap ? a.total : a.dst_cap;
    const long long tiles = (lim + ROWS_IN_TILE - 1) / ROWS_IN_TILE;
    if (tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    a.two_pow = (float)(1ll << (a.bits - 1));
    a.imax = (int32_t)((1ll << (a.bits - 1)) - 1);
    note_launch("k_rows_to_pcm");
    const dim3 grid((unsigned)tiles);
    switch (a.format) {
    case FHIP_ROWS_I32: return launch_fmt<FHIP_ROWS_I32>(st, a, grid);
    case FHIP_ROWS_I16: return launch_fmt<FHIP_ROWS_I16>(st, a, grid);
    default: return launch_fmt<FHIP_ROWS_F32>(st, a, grid);
    }
}

}  // namespace fhip
