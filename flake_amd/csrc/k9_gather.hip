// k9_gather.hip -- K9: a list of spans of channel-interleaved int32 samples, copied from up to two device buffers into
// one destination.  What joins a decode set to an encode set on the device: the decoder's blocks (and each stream's
// carry from the call before) re-cut into the encoder's blocks without the samples leaving the device.
//
// A piece is {src_buf, count, src, dst} in samples per channel; the pieces are sorted by dst and tile [0, total) of the
// destination (the host entry has checked that; the kernel does not rely on it).  Pieces run from one sample to a whole
// block, so the work is dealt out by DESTINATION, not by piece: a workgroup owns one tile of GATHER_TILE_VALS
// interleaved values (4 KiB), a lane the four values of one aligned 16-byte store.  The tile's first and last piece are
// found by two wave-uniform binary searches in the table; a lane then searches only between those two, so a tile
// inside one long piece costs no per-lane search at all and a tile of one-sample pieces log2(1024) steps at most.
//
// A lane whose four values lie in one piece, with a source address that agrees with the destination modulo 16, moves
// them with one 16-byte load; every other lane (a piece boundary inside its four values, 3 channels at an odd offset, a
// source that disagrees) loads value by value.  Stores are 16 bytes except in the destination's last, partial group.
//
// Memory safety is structural, as K7's and K8's: every table index is clamped to [0, npieces), every read into the
// source's declared capacity (a source of capacity 0 is never read), every write lies below both the table's total and
// the destination's capacity -- whatever the device table holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "rows_tile.h"

namespace fhip {
namespace {

constexpr int GATHER_T = 256;                                   // lanes of a workgroup
constexpr int GATHER_LANE_VALS = 4;                             // one 16-byte store
static_assert(GATHER_T * GATHER_LANE_VALS == GATHER_TILE_VALS, "a workgroup covers one tile");

__global__ __launch_bounds__(GATHER_T) void k_gather_spans(GatherArgs a)
{
    // what may be written: below the table's total and the destination's capacity
    const long long ch = a.channels;
    const long long lim_s = a.total < a.dst_cap ? a.total : a.dst_cap;
    const long long lim = lim_s > 0 ? lim_s * ch : 0;
    const long long tile0 = (long long)blockIdx.x * GATHER_TILE_VALS;
    if (tile0 >= lim || a.npieces < 1) return;
    const long long tile_last = (tile0 + GATHER_TILE_VALS < lim ? tile0 + GATHER_TILE_VALS : lim) - 1;
    // wave-uniform: the pieces of the tile's first and last value
    const int last = a.npieces - 1;
    const int p_lo = piece_at(a.pieces, 0, last, tile0 / ch);
    const int p_hi = piece_at(a.pieces, p_lo, last, tile_last / ch);

    const long long v0 = tile0 + (long long)threadIdx.x * GATHER_LANE_VALS;
    if (v0 >= lim) return;
    int pi = p_lo == p_hi ? p_lo : piece_at(a.pieces, p_lo, p_hi, v0 / ch);
    GatherPiece p = a.pieces[pi];
    const int32_t *src = (p.src_buf & 1) ? a.src1 : a.src0;
    long long cap = ((p.src_buf & 1) ? a.src1_cap : a.src0_cap) * ch;      // in values
    long long end = (p.dst + p.count) * ch;                                 // the piece's end in the destination
    long long sv = (p.src - p.dst) * ch + v0;                                // the source value of v0

    int32_t v[GATHER_LANE_VALS] = {0, 0, 0, 0};
    const bool whole = v0 + GATHER_LANE_VALS <= lim;
    if (whole && v0 + GATHER_LANE_VALS <= end && sv >= 0 && sv + GATHER_LANE_VALS <= cap &&
        ((reinterpret_cast<uintptr_t>(src + sv) | reinterpret_cast<uintptr_t>(a.dst + v0)) & 15) == 0) {
        const int4 q = *reinterpret_cast<const int4 *>(src + sv);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < GATHER_LANE_VALS; k++) {
            const long long at = v0 + k;
            if (at >= lim) break;
            // on to the piece that holds this value: pieces are at least one sample long in a table the host took,
            // and the walk ends at the tile's last piece whatever the table holds
            while (at >= end && pi < p_hi) {
                p = a.pieces[++pi];
                src = (p.src_buf & 1) ? a.src1 : a.src0;
                cap = ((p.src_buf & 1) ? a.src1_cap : a.src0_cap) * ch;
                end = (p.dst + p.count) * ch;
            }
            long long s = (p.src - p.dst) * ch + at;
            s = s < 0 ? 0 : (s >= cap ? cap - 1 : s);
            if (cap > 0) v[k] = src[s];
        }
    }
    if (whole && (reinterpret_cast<uintptr_t>(a.dst + v0) & 15) == 0) {
        *reinterpret_cast<int4 *>(a.dst + v0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < GATHER_LANE_VALS; k++)
            if (v0 + k < lim) a.dst[v0 + k] = v[k];
    }
}

}  // namespace

hipError_t launch_gather_spans(hipStream_t st, const GatherArgs &a)
{
    if (a.npieces < 1 || a.total < 1 || a.dst_cap < 1) return hipSuccess;
    const long long lim = (a.total < a.dst_cap ? a.total : a.dst_cap) * (long long)a.channels;
    const long long tiles = (lim + GATHER_TILE_VALS - 1) / GATHER_TILE_VALS;
    note_launch("k_gather_spans");
    hipLaunchKernelGGL(k_gather_spans, dim3((unsigned)tiles), dim3(GATHER_T), 0, st, a);
    return hipGetLastError();
}

}  // namespace fhip
