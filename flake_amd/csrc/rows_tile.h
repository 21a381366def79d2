// rows_tile.h -- what the rows kernels share: K9 (gather), K10 (window rows), K12 (rows in) and K13 (span rows).  Device
// code only, no kernel and no launch: the element type of a rows format and the conversion to it (K10, K12, K13), the
// `in` phase that brings a tile of K7's interleaved samples into LDS (K10, K13), and the bisection of a piece table
// that is sorted by destination (K9, K12).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace fhip {
namespace {

constexpr int ROWS_T = 256;                                     // lanes of a workgroup (K10, K13)
constexpr int ROWS_MAX_CH = 8;
static_assert(ROWS_TILE % 4 == 0, "a channel's line in LDS keeps 16-byte groups");

template <int FMT> struct RowsElem { using type = int32_t; };
template <> struct RowsElem<FHIP_ROWS_I16> { using type = int16_t; };
template <> struct RowsElem<FHIP_ROWS_F32> { using type = float; };

template <int FMT> __device__ inline typename RowsElem<FMT>::type rows_conv(int32_t x, float scale)
{
    if constexpr (FMT == FHIP_ROWS_F32) return (float)x * scale;          // round to nearest even, then an exact scaling
    else if constexpr (FMT == FHIP_ROWS_I16) return (int16_t)x;
    else return x;
}

// in: the span [sv0, sv0 + nvals) of pcm, grouped on the source's 16-byte boundaries, each value into its channel's
// line of `tile` (ROWS_MAX_CH lines of ROWS_TILE values in LDS).  Called by all ROWS_T lanes of the workgroup; the
// caller makes the barrier.  nvals = nt * ch with nt <= ROWS_TILE and ch <= ROWS_MAX_CH; capvals = pcm_cap * ch, and
// every read is clamped into [0, capvals) whatever sv0 is.
__device__ __forceinline__ void rows_tile_load(int32_t *tile, const int32_t *pcm, long long capvals, long long sv0, int nvals, int ch)
{
    const int mis = (int)((reinterpret_cast<uintptr_t>(pcm + sv0) >> 2) & 3);
    const int ngroups = (nvals + mis + 3) >> 2;
    for (int g = threadIdx.x; g < ngroups; g += ROWS_T) {
        const int lo = 4 * g - mis;                                       // the group's first value in the span
        int32_t v[4] = {0, 0, 0, 0};
        const bool whole = lo >= 0 && lo + 4 <= nvals && sv0 + lo + 4 <= capvals;
        if (whole) {
            const int4 q = *reinterpret_cast<const int4 *>(pcm + sv0 + lo);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                long long s = sv0 + lo + j;
                s = s < 0 ? 0 : (s >= capvals ? capvals - 1 : s);
                if (lo + j >= 0 && lo + j < nvals) v[j] = pcm[s];
            }
        }
        int i = (lo < 0 ? 0 : lo) / ch, c = (lo < 0 ? 0 : lo) - i * ch;   // sample and channel of the first value kept
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (lo + j < 0 || lo + j >= nvals) continue;
            tile[c * ROWS_TILE + i] = v[j];                               // (i < nt <= ROWS_TILE, c < ch <= ROWS_MAX_CH)
            if (++c == ch) { c = 0; i++; }
        }
    }
}

// The last piece (in [lo, hi]) whose dst is at or before sample s; lo where none is.  Every index read is in [lo, hi].
template <typename Piece> __device__ inline int piece_at(const Piece *__restrict__ tab, int lo, int hi, long long s)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);              // lo < mid <= hi
        if (tab[mid].dst <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace
}  // namespace fhip
