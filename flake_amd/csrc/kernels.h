// kernels.h -- launch interface between the C ABI (api.hip) and the gfx950
// kernels (k0_prepare.hip ... k6_md5.hip).  Internal to libflakehip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flakehip.h"
#include "flac_header.h"

namespace fhip {

// fhip_last_launches: every launcher notes the kernel instance it queues (template spelling, then
// the runtime switches) into the calling thread's sink, which api.hip sets for the length of an
// encode call.  Host-side only; a no-op while no sink is set.
void note_launch(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
inline const char *tf(bool b) { return b ? "true" : "false"; }

// Blocks up to this size keep a subframe's samples in LDS / registers (K3's k_encode and
// k_encode_pow2); longer ones, up to FHIP_MAX_BLOCK, stream them (k_encode_big).
constexpr int FHIP_MAX_RESIDENT_BLOCK = 16384;

// Everything a launch needs that does not change within a batch.
struct EncodeArgs {
    fhip_params p;
    int n;            // block size of this batch
    int nsub;         // subframes in this batch
};

// A ragged batch (fhip_frames_packed_begin_ragged): blocks of different lengths in one launch.  Frame f has frame_n[f]
// samples per channel and its PCM starts at frame_src[f] (units of the PCM format, as for launch_prepare); frame_c[f]
// is the window constant of lpc.c:34 for that length.  All three are device tables of nframes entries.  Rows of smp,
// the Rice slots and the frame slots keep the stride of row_n (the handle's block size); nmax is the launch's longest
// frame (<= row_n, <= FHIP_MAX_RESIDENT_BLOCK): it sizes LDS and K3's runs, nothing else.  The ragged launchers run the
// generic instances (k_prepare / k_prepare_multi, k_autocorr_ragged, k_encode<C>, k_assemble) with every decision
// the reference derives from the block length taken from the frame's own; K2 takes no length and is launch_lpc.
struct RaggedFrames {
    const int32_t *frame_n;
    const long long *frame_src;
    const double *frame_c;
    int row_n, nmax;
    // optional: the launch's real frame / subframe count lives on the device (the pieces of a ragged variable-block-size
    // batch, k_vbs_plan_ragged); nframes / nsub then size the grid, and a workgroup or wave at or past the count leaves
    // before it reads a table entry.  Null: the launch as it was.
    const int32_t *dev_frames = nullptr, *dev_sub = nullptr;
};
hipError_t launch_prepare_ragged(hipStream_t st, const fhip_params &p, const int32_t *pcm, int nframes,
                                 const RaggedFrames &rf, int32_t *smp, fhip_subframe_info *info, int pcm_format);
hipError_t launch_autocorr_ragged(hipStream_t st, const int32_t *smp, int nsub, int nch, const RaggedFrames &rf,
                                  int max_order, double *autoc);
hipError_t launch_encode_ragged(hipStream_t st, const fhip_params &p, const int32_t *smp, int nsub,
                                const RaggedFrames &rf, const int32_t *coefs, const int32_t *shift,
                                const int32_t *opt_order, fhip_subframe_info *info, uint8_t *bits, int64_t slot_bytes,
                                const fhip_subframe_info *prep);

// K0: copy_samples + channel_decorrelation + remove_wasted_bits
// (encode.c:541-694).  pcm [nframes][n][ch] -> smp [nframes][ch][n].
// decide_only: write obits / wasted / ch_mode to info[] and leave smp to the fused K1.
// allow_narrow: a channel whose samples all fit 16 bits is stored as int16[n] at the
// start of its row and flagged in info.reserved (see narrow_rows_ok).
// frame_src (optional): frame f's PCM starts at pcm + frame_src[f] (int32 units) instead of
// pcm + f*n*ch -- the pieces of a variable-block-size batch are encoded where they lie.
// dev_frames / dev_sub (optional, every launch_* below): the launch's real frame / subframe count
// lives on the device; nframes / nsub then size the grid (the bin's capacity) and workgroups past
// the count leave at once (device_util.h: dev_count).
// pcm_format (FHIP_PCM_*): with FHIP_PCM_S16, pcm addresses interleaved int16 (the k_*_s16 instances; bits_per_sample
// <= 16, no decide_only) and frame_src counts int16 units.  K4 and K5 take the format the same way.
hipError_t launch_prepare(hipStream_t st, const fhip_params &p, const int32_t *pcm,
                          int nframes, int n, int32_t *smp, fhip_subframe_info *info,
                          bool decide_only = false, bool allow_narrow = false,
                          const long long *frame_src = nullptr, const int32_t *dev_frames = nullptr,
                          int pcm_format = FHIP_PCM_S32);

// True when K0, K1 and K3 all handle 16-bit sample rows for such a batch; the
// caller then passes allow_narrow / narrow_ok to the three launches of the batch.
// (wave_typed_k1: the caller runs the wave-typed K1 whatever the count -- launch_autocorr_bins)
bool narrow_rows_ok(const fhip_params &p, int nsub, int n, bool lpc_path, bool wave_typed_k1 = false);

// True when K1 will also do K0's apply stage for such a batch (stereo, whole
// tiles, the wave-typed kernel): launch_prepare(decide_only) + launch_autocorr(pcm).
bool autocorr_fuses_prepare(const fhip_params &p, int nsub, int n);

// The wave-typed K1: a workgroup owns WT_SUB subframes, and its four producer waves stage rows[0..3] of them
// each, in row order (producer p starts at the prefix sum wt_split_first(s, p)).  Counts are even (the fused
// instances stage channel pairs) and positive, and they sum to WT_SUB, so every row is staged exactly once.
constexpr int WT_SUB = 32;
struct wt_split { int rows[4]; };
constexpr int wt_split_first(const wt_split &s, int p)
{
    int q = 0;
    for (int k = 0; k < p; k++) q += s.rows[k];
    return q;
}
constexpr bool wt_split_valid(const wt_split &s)
{
    for (int k = 0; k < 4; k++) if (s.rows[k] < 2 || (s.rows[k] & 1)) return false;
    return wt_split_first(s, 4) == WT_SUB;
}
// true when no producer before p has p's row count (one instance of the staging code per distinct count)
constexpr bool wt_split_first_with(const wt_split &s, int p)
{
    for (int k = 0; k < p; k++) if (s.rows[k] == s.rows[p]) return false;
    return true;
}
// FHIP_WT_ROWS_P0 .. _P3: the split of k_autocorr_wt<3, false, 8> (max order 8, unsplit: the headline's K1),
// one build constant per producer (-DFHIP_WT_ROWS_P0=6 -DFHIP_WT_ROWS_P1=12 ... for timing another split);
// every other instance stages 8/8/8/8 (k1_autocorr.hip: wt_split_of).
#ifndef FHIP_WT_ROWS_P0
#define FHIP_WT_ROWS_P0 8
#endif
#ifndef FHIP_WT_ROWS_P1
#define FHIP_WT_ROWS_P1 8
#endif
#ifndef FHIP_WT_ROWS_P2
#define FHIP_WT_ROWS_P2 8
#endif
#ifndef FHIP_WT_ROWS_P3
#define FHIP_WT_ROWS_P3 8
#endif
constexpr wt_split WT_SPLIT_EVEN = {{8, 8, 8, 8}};
constexpr wt_split WT_SPLIT_O8 = {{FHIP_WT_ROWS_P0, FHIP_WT_ROWS_P1, FHIP_WT_ROWS_P2, FHIP_WT_ROWS_P3}};
static_assert(wt_split_valid(WT_SPLIT_EVEN) && wt_split_valid(WT_SPLIT_O8), "producer row split");

// K1: apply_welch_window + compute_autocorr (lpc.c:28-71).
// smp [nsub][n] -> autoc [nsub][FHIP_MAX_LAGS].
// With pcm_fused (stereo PCM) the producers read it instead of smp, apply info[]'s
// channel mode / wasted bits and write smp_out.
// With lpc_out (see autocorr_does_lpc) the kernel also does K2's work for its
// subframes and launch_lpc is not needed.
// tile_ctr (optional): one arrival counter per tile of 32 subframes, zeroed once (fhip_create) -- with it a
// lag-split launch (small batches: two workgroups per tile) still runs K2 as its tail, in whichever of a tile's
// two workgroups arrives second (the counters run on, their parity tells the arrivals apart).
struct autocorr_lpc_out { int precision, omethod; int32_t *coefs, *shift, *opt_order, *fin; int32_t *tile_ctr = nullptr; };
bool autocorr_does_lpc(int nsub, int n, int max_order, bool have_tile_counters = false);
// True when the wave-typed K1 (k_autocorr_wt) serves such a batch.
bool autocorr_is_wave_typed(int nsub, int n, int max_order);
hipError_t launch_autocorr(hipStream_t st, const int32_t *smp, int nsub, int n,
                           int max_order, double *autoc, const int32_t *pcm_fused = nullptr,
                           int32_t *smp_out = nullptr, const fhip_subframe_info *info = nullptr,
                           const autocorr_lpc_out *lpc_out = nullptr, bool narrow_ok = false,
                           const int32_t *dev_sub = nullptr, int nsub_hint = 0);

// K2: compute_lpc_coefs / _est + quantize_lpc_coefs (lpc.c:77-257).
// coefs [nsub][32][32], shift [nsub][32], opt_order [nsub].
// fin [nsub][FIN_STRIDE]: for the MAX/EST order methods the one row the
// reference quantises, compact: coefs[0..32), shift, order (prefetched by K3).
constexpr int FIN_STRIDE = 72;      // int32 per row: 32 coefs, shift, order, sum|coef|, 1 spare,
constexpr int FIN_DBL = 36;         // ... the first 16 coefficients once more as doubles (zero past the order:
                                    //     K3 reads them by scalar loads, they never touch a vector register),
constexpr int FIN_PAIRS = 68;       // ... and the first 8 as four int16 pairs (lo: tap 2j+2, hi: tap 2j+1)
hipError_t launch_lpc(hipStream_t st, const double *autoc, int nsub, int max_order,
                      int precision, int omethod, int32_t *coefs, int32_t *shift,
                      int32_t *opt_order, int32_t *fin, const int32_t *dev_sub = nullptr);

// prep: the records K0 filled (obits, wasted, ch_mode, the 16-bit-row flag) -- the handle's
// own buffer, never info[] itself (the kernels' pointers to the two are __restrict__); K3
// copies K0's fields from there into info[].
// K3: encode_residual (optimize.c:124-276) incl. the Rice search (rice.c) and,
// when bits != NULL, the residual section of output_residual (encode.c:766-798).
hipError_t launch_encode(hipStream_t st, const fhip_params &p, const int32_t *smp,
                         int nsub, int n, const int32_t *coefs, const int32_t *shift,
                         const int32_t *opt_order, const int32_t *fin,
                         fhip_subframe_info *info,
                         int32_t *residual, uint8_t *bits, int64_t slot_bytes,
                         int raw_order = -1, int raw_lpc = 0, bool narrow_ok = false,
                         const fhip_subframe_info *prep = nullptr, bool order_known = false,
                         const int32_t *dev_sub = nullptr);

// K3-S: the LPC order searches (order methods 2..6, optimize.c:201-261) for block sizes it
// supports: bits[order] for every order the method can visit, the method's walk over that
// table, and the winner left as K2 leaves the single row of MAX / EST (opt_order[s], fin[s]);
// launch_encode(..., order_known = true) then encodes it with the lean instance.
bool order_search_supported(const fhip_params &p, int n);
hipError_t launch_order_search(hipStream_t st, const fhip_params &p, const int32_t *smp, int nsub,
                               int n, const int32_t *coefs, const int32_t *shift,
                               int32_t *opt_order, int32_t *fin, const fhip_subframe_info *prep,
                               bool narrow_ok, const int32_t *dev_sub = nullptr,
                               uint32_t *table_out = nullptr);

struct MultiBin;
// The thinly filled bins of a small ragged batch: several bins in one search launch and one K3 launch.
// order_search_group: >= 0, equal for bins that can share a launch (-1: launch_order_search for that bin alone);
// encode_group: 256 or -1 likewise.  mb: units = subframes, wg0 from the capacities, cnt = live subframes per bin, unit0 =
// the bin's first subframe, smp_off, narrow (+ slot, bits_off for K3); the workspaces whole.
int order_search_group(const fhip_params &p, int n);
hipError_t launch_order_search_bins(hipStream_t st, const fhip_params &p, const MultiBin &mb, const int32_t *smp,
                                    const int32_t *coefs, const int32_t *shift, int32_t *opt_order, int32_t *fin,
                                    const fhip_subframe_info *prep);
int encode_group(const fhip_params &p, int n, bool order_known);
hipError_t launch_encode_bins(hipStream_t st, const fhip_params &p, const MultiBin &mb, const int32_t *smp,
                              const int32_t *coefs, const int32_t *shift, const int32_t *opt_order, const int32_t *fin,
                              fhip_subframe_info *info, const fhip_subframe_info *prep, uint8_t *bits);

// K4: whole frames on the device (encode.c:718-764, :800-917, :949-964):
// frames [nframes][frame_stride] bytes, frame_bytes [nframes].
hipError_t launch_assemble(hipStream_t st, const fhip_params &p, const int32_t *pcm, int nframes,
                           int n, const fhip_subframe_info *info, const uint8_t *rice,
                           int64_t slot_bytes, uint8_t *frames, int64_t frame_stride,
                           int32_t *frame_bytes, uint32_t number_base, uint32_t number_step,
                           const uint32_t *numbers = nullptr, const long long *frame_src = nullptr,
                           const int32_t *dev_frames = nullptr, int pcm_format = FHIP_PCM_S32,
                           const int32_t *frame_n = nullptr);       // frame_n (with frame_src): the ragged instance

// K4-P: offsets[f] = exclusive scan of frame_bytes (offsets[nframes] = total) and the frames
// copied back to back into packed[] -- the stream order flake_encode_frame's callers write.
hipError_t launch_pack_frames(hipStream_t st, const uint8_t *frames, int64_t frame_stride,
                              const int32_t *frame_bytes, int nframes, long long *offsets,
                              uint8_t *packed);

// Ragged (VBS) batches on the device (k4_assemble.hip).  A piece is k eighths of its block: eight
// bins of equal piece length, bin k-1 with a fixed range of frame slots for the most pieces it
// can get (floor(8 / k) per block).  Host constants per bin:
struct VbsBins {
    int n[8];                 // piece length k * block_size / 8
    int cap[8];               // frame slots: floor(8 / k) * nblocks
    int slot0[8];             // first frame slot (subframe-indexed workspaces: slot0 * channels)
    long long smp_off[8];     // first sample of the bin's rows in smp[] (int32 units)
    long long stride[8];      // fhip_frame_stride of the piece length
    long long fr_off[8];      // byte offset of the bin's frames in frames[]
    long long slot[8];        // residual-section slot bytes of the piece length
    long long bits_off[8];    // byte offset of the bin's sections in rice_bits[]
};
// One launch over ALL bins for the kernels whose code does not depend on the piece length (K1's
// wave-typed kernel, K2, K4): the chain walk of K1, the Levinson recursion of K2 and the serial
// header / CRC phases of K4 are latency, not throughput, and eight launches of a few hundred
// frames each paid it eight times.  Workgroup -> (bin, unit inside the bin) through wg0[]; the
// unit-indexed arrays (info, autoc, coefs ...) are the handle's whole workspaces, indexed by
// unit0[bin] + local unit; sample rows start at smp_off[bin].
struct MultiBin {
    int nbins;                // 0: a plain launch
    const int32_t *cnt;       // device: live units (subframes for K1 / K2, frames for K4) of entry k at
    int cnt_ix[8];            //   cnt[cnt_ix[k]]: entries may list the bins in any order (K1: longest first)
    int wg0[9];               // first workgroup of bin k; wg0[nbins] = the grid
    int n[8];
    int unit0[8];             // K1 / K2: first subframe of the bin; K4: first frame slot
    int cap[8];               // units the bin can hold
    int narrow[8];            // K1: the bin's rows may be 16-bit (K0's records say which)
    long long smp_off[8];
    double c[8];              // K1: the window constant of lpc.c:34 for the bin's n
    long long stride[8], fr_off[8], slot[8], bits_off[8];     // K4
    int vsize[8];                                              // K4: verbatim size (encode.c:521-527)
};
// K0 over all bins of a stereo batch (unit0 = first frame slot of the bin, cnt = live frames, wg0 from
// prepare_bins_workgroups): frame_src[slot] = the piece's offset in pcm
bool prepare_bins_supported(const fhip_params &p, const int *n, int nbins);
int prepare_bins_workgroups(int n, int cap, int nmax);     // nmax: the batch's longest bin
hipError_t launch_prepare_bins(hipStream_t st, const fhip_params &p, const int32_t *pcm, const MultiBin &mb,
                               int32_t *smp, fhip_subframe_info *info, const long long *frame_src);
hipError_t launch_autocorr_bins(hipStream_t st, const MultiBin &mb, const int32_t *smp, int max_order,
                                double *autoc, const fhip_subframe_info *info,
                                const autocorr_lpc_out *lpc_out);
bool autocorr_bins_supported(int max_order, const int *n, int nbins);
hipError_t launch_lpc_bins(hipStream_t st, const MultiBin &mb, const double *autoc, int max_order,
                           int precision, int omethod, int32_t *coefs, int32_t *shift,
                           int32_t *opt_order, int32_t *fin);
hipError_t launch_assemble_bins(hipStream_t st, const fhip_params &p, const MultiBin &mb, const int32_t *pcm,
                                const fhip_subframe_info *info, const uint8_t *rice, uint8_t *frames,
                                int32_t *frame_bytes, const uint32_t *numbers, const long long *frame_src);

// CNT_*: layout of the device-side counts k_vbs_plan leaves (int32[24])
constexpr int VBS_CNT_FRAMES = 0, VBS_CNT_SUB = 8, VBS_CNT_ALL = 16, VBS_CNT_WORDS = 24;
hipError_t launch_vbs_plan(hipStream_t st, const int32_t *nfr, const int32_t *sizes, int nblocks,
                           int block_size, int nch, uint32_t first_number, const VbsBins &bins,
                           int32_t *cnt, int32_t *order, long long *frame_src, long long *src_off,
                           uint32_t *numbers, int32_t *first, const uint32_t *block_first = nullptr);
// (block_first, optional device [nblocks]: the blocks of many streams -- block b's pieces are numbered from
// block_first[b] instead of first_number + the block's offset in the batch)
// The frames of all bins packed in stream order: order[i] = slot of the stream's i-th frame,
// src_off[slot] = byte offset of that slot's frame in frames[] (4-byte aligned), *dev_frames of them
// (<= max_frames); offsets[i] / offsets[count] as in launch_pack_frames; stream_bytes[i] (optional)
// = size of the stream's i-th frame; totals[4] = {frames, bytes, largest frame, stream > cap}.
hipError_t launch_pack_frames_perm(hipStream_t st, const uint8_t *frames, const long long *src_off,
                                   const int32_t *frame_bytes, const int32_t *order, int max_frames,
                                   const int32_t *dev_frames, long long *offsets, uint8_t *packed,
                                   long long cap, int32_t *stream_bytes, long long *totals);
hipError_t launch_vbs_block_bytes(hipStream_t st, const int32_t *first, const long long *offsets, int nblocks,
                                  int32_t *block_bytes, int32_t *block_frames,
                                  int32_t *block_max_frame = nullptr);    // optional: block b's largest frame

// K-vbs: split_frame_v1 (vbs.c:36-83) for nblocks blocks: nframes_out [nblocks],
// sizes_out [nblocks][8].
hipError_t launch_vbs_split(hipStream_t st, const int32_t *pcm, int nblocks, int block_size,
                            int nch, int32_t *nframes_out, int32_t *sizes_out);

// The same for blocks of DIFFERENT lengths (the tails of many streams): block b is block_n[b] samples at block_src[b]
// (interleaved values into pcm; device tables).  A block with n % 8 == 0 && n >= 128 is scored and cut as above (the
// eighth is n / 8); any other is one piece (encode.c:997-999): nframes 1, sizes {n, 0 ...}.
hipError_t launch_vbs_split_ragged(hipStream_t st, const int32_t *pcm, int nblocks, const int32_t *block_n,
                                   const long long *block_src, int nch, int32_t *nframes_out, int32_t *sizes_out);
// The piece tables of such a batch, dense and in stream order (piece i of the batch = the i-th frame of the stream of
// frames): frame_n / frame_src / frame_c as RaggedFrames takes them, numbers[i] = block_first[b] + the piece's offset in
// its block (uint32 wrap), first[b] = index of block b's first piece (first[nblocks] = pieces in all), cnt[0] / cnt[1] =
// live pieces / subframes.  block_c [nblocks][8]: the window constant of lpc.c:34 for m eighths of block b at [m - 1]
// (the whole block at [7], whatever its length), computed on the host; the kernel picks, it never divides.  All `cap`
// (= 8 * nblocks) slots of the piece tables are written -- the dead ones as one-sample pieces at offset 0 -- and
// order[i] = i, src_off[i] = i * frame_stride, so that launch_pack_frames_perm packs the slots as they lie.
hipError_t launch_vbs_plan_ragged(hipStream_t st, const int32_t *nfr, const int32_t *sizes, int nblocks,
                                  const int32_t *block_n, const long long *block_src, const double *block_c,
                                  const uint32_t *block_first, int nch, long long frame_stride, int32_t *cnt,
                                  int32_t *frame_n, long long *frame_src, double *frame_c, uint32_t *numbers,
                                  int32_t *first, int32_t *order, long long *src_off);

// Dynamic-LDS need of K3 for a block size (0 if unsupported).
size_t encode_lds_bytes(int n);

// Fast-path geometry of K3 for a block size: C samples per thread, T threads, n = C*T.
bool fast_geometry(const fhip_params &p, int n, int *C, int *T);

// K5 (k5_verify.hip): does each frame of a stream decode to the caller's PCM?  Reads the stream, the
// frame sizes, the PCM and the parameters below -- no encoder intermediate.  Three launches on st:
// k_verify_frames (one workgroup: offsets, headers, numbering; fills ws[] and zeroes the summary),
// k_verify (a workgroup per frame), k_verify_final (summary[2..3]; totals[3] |= 4 when a frame failed).
struct VerifyFrame {
    long long off;          // byte offset of the frame in the stream
    long long rel_start;    // its first sample, as an index into pcm
    long long bit;          // status != OK: bit of the first discrepancy
    int bytes, n, hdr_bits, ch_code, status;
};
struct VerifyArgs {
    const uint8_t *stream; long long stream_bytes;
    const int32_t *frame_bytes; int nframes;      // nframes: the grid (and the count when dev_count is null)
    const long long *dev_count;                  // optional: the real frame count lives on the device
    const int32_t *pcm; long long nsamples; long long first_sample;
    int channels, bps, block_size, sample_rate, allow_vbs;
    int pcm_format;                              // FHIP_PCM_*: S16 = pcm addresses int16
    VerifyFrame *ws;                             // [nframes]
    fhip_verify_rec *recs;                       // optional [nframes]
    long long *summary;                          // [4]
    unsigned long long *key;                     // [1] scratch: (first failing frame << 8) | status
    long long *totals;                           // optional: fhip_encode_blocks_vbs_dev's totals
    const uint32_t *numbers;                     // optional [nframes], fixed blocks only: the number frame f must carry
                                                 // (frames of many streams in one batch); first_sample is unused then
    const int32_t *frame_n = nullptr;            // optional, with numbers (the ragged numbered mode): frame f must hold exactly
    const long long *frame_src = nullptr;        // frame_n[f] samples, found at frame_src[f] of pcm (units of the PCM format)
    // The block-table mode (allow_vbs only; without the table every launch is the sequence mode's): the batch is nblocks
    // blocks of block_size samples, each of some stream and of one or more frames; where a frame lies follows from the
    // header-parsed sizes of the frames before it (a scan), and a frame at offset `off` of block b must carry
    // block_first[b] + off.  first_sample is unused then.
    const uint32_t *block_first = nullptr;       // optional [nblocks]
    int nblocks = 0;
    // ... with a length per block: block b covers samples block_start[b] .. block_start[b + 1] of the batch (prefix sums,
    // [nblocks + 1]); a frame's block is found by search (vbs_block_lookup.h) where the uniform mode divides
    const long long *block_start = nullptr;
};
hipError_t launch_verify(hipStream_t st, const VerifyArgs &a);

// K7 (k7_decode.hip): a batch of frames back to PCM, by the format alone.  Three launches on st, as K5's:
// k_decode_frames (one workgroup: offsets, headers, where each frame's samples go, numbering; fills ws[], zeroes the
// summary, leaves the sample count), k_decode (a wave per frame), k_decode_final (summary[2..3]).
struct DecodeArgs {
    const uint8_t *stream; long long stream_bytes;
    const int32_t *frame_bytes; int nframes;
    int variable_blocks;                         // the blocking-strategy bit every header must carry: 1 = sample numbers
    long long first_number;                      // the number frame 0 must carry; < 0: only continuity is checked
    int channels, bps, block_size, sample_rate;  // the handle's: header codes are held against them; block_size is
                                                 // the largest block accepted and the stride of rows
    int pcm_format;                              // FHIP_PCM_*: S16 = pcm addresses int16
    void *pcm; long long pcm_cap;                // interleaved output, pcm_cap samples per channel
    int32_t *rows;                               // [nframes][channels][block_size] restored subframes (the handle's d_smp)
    VerifyFrame *ws;                             // [nframes]
    fhip_verify_rec *recs;                       // optional [nframes]
    long long *summary;                          // [4]
    unsigned long long *key;                     // [1] scratch: (first failing frame << 8) | status
    long long *nsamples;                         // [1] samples per channel of the frames whose header pass succeeded
    long long *written_end;                      // [1] where the last of those frames ends in pcm (samples per channel):
                                                 // nothing at or behind it is written
    // The segment mode (null seg_first: every launch is as it was): the batch is nsegs runs of consecutive frames, each
    // of one stream -- segment s is frames seg_first[s] .. seg_first[s + 1] (CSR, [nsegs + 1], 0 .. nframes, a frame's
    // segment is found by search).  Numbering, the size rule of fixed blocks and the strategy bit are held per segment:
    // variable_blocks and first_number above are unused.  Placement stays the batch's.  recs is required then: the
    // segment pass of the end reads the frames' final statuses from it.
    const int32_t *seg_first = nullptr;
    int nsegs = 0;
    const long long *seg_number = nullptr;       // [nsegs] the number the segment's first frame must carry; < 0: not checked
    const int32_t *seg_variable = nullptr;       // [nsegs] the strategy bit of the segment's headers
    long long *seg_start = nullptr;              // [nsegs] out: where the segment's samples begin in pcm
    long long *seg_samples = nullptr;            // [nsegs] out: as nsamples, of the segment's frames
    int32_t *seg_failed = nullptr;               // [nsegs] out: index in the batch of its first failing frame, -1: none
};
hipError_t launch_decode(hipStream_t st, const DecodeArgs &a);
// k_decode_final and, in the segment mode, k_decode_seg_final: the end of launch_decode and of launch_decode_windows.
hipError_t launch_decode_end(hipStream_t st, const DecodeArgs &a);

// K7's window mode (k7_decode_windows.hip): the segment mode, of which every table of d is required, with a window of
// samples per segment.  A frame whose samples are [o, o + n) of its segment -- o the sizes of the segment's good headers
// before it -- delivers [max(o, skip), min(o + n, skip + take)), and what the batch delivers lies back to back in pcm:
// seg_start, seg_samples, nsamples, written_end and pcm_cap are about the delivered samples.  Every frame is decoded
// and checked in full.  The header pass leaves each frame's clip in clip[], which the frame pass writes out by.  Both
// are the window instances of k7_frame.h's passes, of which k7_decode.hip's kernels are the others.
// Launches: "k_decode_frames windows", "k_decode windows", then launch_decode_end's.
struct DecodeClip {
    long long dst;          // where the clip's first sample goes in pcm
    int lo, cnt;            // the clip: samples lo .. lo + cnt of the frame (cnt 0: nothing)
};
struct DecodeWindowArgs {
    DecodeArgs d;
    const long long *seg_skip;                   // [nsegs] samples to drop from the segment's front (below 0: 0)
    const long long *seg_take;                   // [nsegs] the most to deliver behind them; < 0: to the segment's end
    DecodeClip *clip;                            // [nframes] workspace
};
hipError_t launch_decode_windows(hipStream_t st, const DecodeWindowArgs &w);

// K6 (k6_md5.hip): the STREAMINFO MD5 of many streams, one lane per stream.  The update hashes, for stream s, the
// blocks seg_block[seg_first[s] .. seg_first[s + 1]) -- indices of block_vals-sample blocks (block_size * channels
// interleaved values) of pcm -- in that order.  pcm_format as for K0; bytes_per_sample = (bits_per_sample + 7) / 8.
// The fast path needs md5_shape_fast() (whole 64-byte blocks per PCM block, 16-byte aligned) AND no stream of the
// launch holding a partial block: the second is only known on the device, so a shape-fast launch is preceded by
// k_md5_scan, which leaves the answer in flag[0] (device) and host_flag[0] (pinned host memory, optional).
bool md5_shape_fast(int block_vals, int bytes_per_sample, int pcm_format, const void *pcm);
hipError_t launch_md5_init(hipStream_t st, fhip_md5_state *states, int nstreams);
hipError_t launch_md5_streams(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm, int pcm_format,
                              int block_vals, int bytes_per_sample, const int32_t *seg_first,
                              const int32_t *seg_block, int32_t *flag, int32_t *host_flag, bool *shape_fast_out);
// The general path over blocks given as (offset, length) pairs: block b is the blk_vals[b] interleaved values at
// pcm + blk_off[b] (units of the PCM format); seg_block indexes those tables.
hipError_t launch_md5_streams_ragged(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm,
                                     int pcm_format, int bytes_per_sample, const int32_t *seg_first,
                                     const int32_t *seg_block, const long long *blk_off, const int32_t *blk_vals);
// The update over ranges of samples that the device names (k_md5_ranges): stream s absorbs the ranges
// seg_range[seg_first[s] .. seg_first[s + 1]) in order; range r is range_samples[r] samples per channel (<= 0: nothing)
// at sample range_start[r] of pcm.  Both tables are device int64 -- in a decode set K7's seg_start / seg_samples.  Any
// fill, any length, any sample-aligned start: whole units go through registers, the ends through the tail.
hipError_t launch_md5_ranges(hipStream_t st, fhip_md5_state *states, int nstreams, const void *pcm, int pcm_format,
                             int bytes_per_sample, int channels, const int32_t *seg_first, const int32_t *seg_range,
                             const long long *range_start, const long long *range_samples);
hipError_t launch_md5_final(hipStream_t st, const fhip_md5_state *states, int nstreams, uint8_t *digests);

// K8 (k8_index.hip): frame discovery, the CPU indexer's answer for nranges streams at once.  INDEX_STEPS launches on st,
// one per launch_index_step so that the caller can time each: the candidate pass (count), the scan over its
// workgroups, the candidate pass again (scatter), the walk (a wave per range), the ranges' places, the sizes.
struct IndexArgs {
    const uint8_t *stream; long long stream_bytes;
    const long long *range_first; int nranges;   // [nranges + 1]; read clamped into the stream
    flac_format fmt;                             // what the header codes are held against (max_block_size 0: not checked)
    long long frame_cap;
    int32_t *frame_bytes, *range_frames; long long *range_consumed; int32_t *range_variable;
    // working memory (the handle's)
    int nwg;                                     // index_nwg(stream_bytes): the candidate pass's workgroups
    int32_t *wg_cnt;                             // [nwg] candidates per workgroup, then their exclusive prefix
    uint32_t *wg_key;                            // [nwg + 1] key terms per workgroup, then the key at each one's first byte
    int32_t *ncand;                              // [1] candidates found (may exceed table_cap: the table keeps the first)
    long long table_cap;                         // entries of the four candidate arrays
    int32_t *cand_pos; uint32_t *cand_meta; unsigned long long *cand_numkey;
    int32_t *cand_end;                           // the walk's frame ends, from the range's first table index on
    int32_t *rng_cf, *rng_cnt, *rng_vbs; long long *rng_off;     // [nranges] each
};
constexpr int INDEX_STEPS = 6;
const char *index_step_name(int step);
int index_nwg(long long stream_bytes);
void index_geometry(int *lane_bytes, int *wg_bytes, int *end_lane_bytes, int *xinv8);
hipError_t launch_index_step(hipStream_t st, const IndexArgs &a, int step);

// K9 (k9_gather.hip): spans of channel-interleaved int32 samples from up to two sources into one destination.  One
// launch on st, a workgroup per GATHER_TILE_VALS interleaved values of the destination (4 KiB).  pieces is a DEVICE
// table, sorted by dst and tiling [0, total); every read of it is clamped to [0, npieces), every source read into
// [0, srcN_cap) and every write below min(total, dst_cap) samples, whatever it holds.
using GatherPiece = fhip_gather_piece;
struct GatherArgs {
    int32_t *dst; long long dst_cap;             // capacities in samples per channel
    const int32_t *src0; long long src0_cap;
    const int32_t *src1; long long src1_cap;
    const GatherPiece *pieces; int npieces;
    long long total;                             // the samples per channel the table covers
    int channels;
};
constexpr int GATHER_TILE_VALS = 1024;
hipError_t launch_gather_spans(hipStream_t st, const GatherArgs &a);

// K10 (k10_rows.hip): the segments K7's window mode left interleaved in pcm, as rows[nrows][channels][row_len] of int32,
// int16 or float32 (format: FHIP_ROWS_*).  One launch on st, a workgroup per segment and tile of ROWS_TILE samples, sized
// for the longest segment there can be.  All five tables are DEVICE memory; every read of them is clamped to
// [0, nsegs), every source read into [0, pcm_cap * channels) and every write into the row's own [0, row_len) of a row in
// [0, nrows), whatever they hold.  Segment k is delivered when seg_failed[k] < 0 and its row, column and start are in
// range, cut at the row's end and at pcm_cap.  Nothing else is written.
struct WindowRowsArgs {
    const int32_t *pcm; long long pcm_cap;       // K7's interleaved output, samples per channel
    int nsegs;
    const long long *seg_start, *seg_samples;    // [nsegs] as K7 left them
    const int32_t *seg_failed;                   // [nsegs]
    const int32_t *seg_row;                      // [nsegs] the destination row; outside [0, nrows): not delivered
    const long long *seg_col;                    // [nsegs] the first column
    void *rows; int nrows; long long row_len;
    int format, channels;
    float scale;                                 // FHIP_ROWS_F32: 2^-(bits_per_sample - 1)
    int tiles = 0;                               // (the launch's: tiles per segment)
};
constexpr int ROWS_TILE = 512;
hipError_t launch_window_rows(hipStream_t st, const WindowRowsArgs &a);

// K13 (k13_span_rows.hip): K10 one to many -- a segment is a run of a SPAN whose samples go into every row of row_len
// samples, hop apart, that they belong to: sample i of segment k is at span position p = seg_pos[k] + i and is written
// to column p - j * hop of row seg_row0[k] + j for every j in [0, seg_nrows[k]) with j * hop <= p < j * hop + row_len.
// One launch on st of ntiles workgroups, a workgroup per segment and tile of ROWS_TILE samples: tile_first [nsegs + 1]
// is the CSR of the tiles the caller allots each segment (from an upper bound of its length; samples behind a
// segment's tiles are not delivered).  All seven tables are DEVICE memory; every read of them is clamped to
// [0, nsegs), every source read into [0, pcm_cap * channels) and every write into the own [0, row_len) of a row in
// [seg_row0, seg_row0 + seg_nrows), itself in [0, nrows), whatever they hold.  Segment k is delivered when
// seg_failed[k] < 0, seg_nrows[k] >= 1, its rows lie in [0, nrows), seg_pos[k] >= 0 and its start is in range, cut at
// pcm_cap.  Nothing else is written.
struct SpanRowsArgs {
    const int32_t *pcm; long long pcm_cap;       // K7's interleaved output, samples per channel
    int nsegs;
    const long long *seg_start, *seg_samples;    // [nsegs] as K7 left them
    const int32_t *seg_failed;                   // [nsegs]
    const int32_t *seg_row0, *seg_nrows;         // [nsegs] the span's first row and its rows
    const long long *seg_pos;                    // [nsegs] the span position of the segment's first delivered sample
    const int32_t *tile_first; int ntiles;       // [nsegs + 1] from 0 to ntiles, not decreasing
    void *rows; int nrows; long long row_len, hop;
    int format, channels;
    float scale;                                 // FHIP_ROWS_F32: 2^-(bits_per_sample - 1)
};
hipError_t launch_span_rows(hipStream_t st, const SpanRowsArgs &a);

// K12 (k12_rows_in.hip): K10's inverse -- spans of rows[nrows][channels][row_len] (int32, int16 or float32; format:
// FHIP_ROWS_*) converted and laid channel-interleaved as int32 into dst.  One launch on st, a workgroup per ROWS_IN_TILE
// samples of the destination.  pieces is a DEVICE table, sorted by dst and tiling [0, total); every read of it is
// clamped to [0, npieces), every row to [0, nrows), every column to [0, row_len) and every write below
// min(total, dst_cap) samples, whatever it holds.  float32: x = clamp(rne(e * 2^(bits-1))), NaN -> 0.
using RowPiece = fhip_row_piece;
struct RowsInArgs {
    int32_t *dst; long long dst_cap;             // capacity in samples per channel
    const void *rows; int nrows; long long row_len;
    const RowPiece *pieces; int npieces;
    long long total;                             // the samples per channel the table covers
    int channels, format, bits;                  // bits: the handle's bits_per_sample
    float two_pow = 0.f; int32_t imax = 0;       // (the launch's: 2^(bits-1) and 2^(bits-1) - 1)
};
constexpr int ROWS_IN_TILE = 1024;
hipError_t launch_rows_to_pcm(hipStream_t st, const RowsInArgs &a);

// K11 (k11_held.hip): frames of a store that stays on the device.  All tables are DEVICE memory.
// k_frame_heads: heads[f] is flac_header_ok(fmt, stream + frame_off[f], frame_bytes[f]) as a record, all zero where it
// answers 0, where frame_bytes[f] <= 0 and where the frame's range leaves [0, stream_bytes).  One lane per frame.
struct FrameHeadsArgs {
    const uint8_t *stream; long long stream_bytes;
    const long long *frame_off; const int32_t *frame_bytes; long long nframes;
    flac_format fmt;
    fhip_frame_head *heads;                      // [nframes]
};
hipError_t launch_frame_heads(hipStream_t st, const FrameHeadsArgs &a);
// k_frame_offsets: K8's answers (frame_bytes back to back in range order, range_frames) turned into the table
// k_frame_heads reads: frame_off[f] = base + range_first[r] + the sizes of range r's frames before f.  A wave per range;
// nothing at or past frame_cap is read or written.
struct FrameOffsetsArgs {
    const long long *range_first; const int32_t *range_frames; int nranges;
    const int32_t *frame_bytes; long long frame_cap;
    long long base;
    long long *frame_off;                        // [frame_cap]
};
hipError_t launch_frame_offsets(hipStream_t st, const FrameOffsetsArgs &a);
// k_gather_offsets (one workgroup), then k_gather_frames (a wave per frame): frame f is accepted when frame_len[f] >= 1,
// [frame_src[f], frame_src[f] + frame_len[f]) lies inside [0, src_bytes) and its place -- the accepted lengths before it,
// added up -- fits dst_cap.  An accepted frame is copied to its place and dst_frame_bytes[f] is its length; any other
// gets 0 and copies nothing.  No read outside [0, src_bytes), no write outside the frame's own range of [0, dst_cap).
struct GatherFramesArgs {
    uint8_t *dst; long long dst_cap;
    int32_t *dst_frame_bytes;                    // [nframes]
    const uint8_t *src; long long src_bytes;
    const long long *frame_src; const int32_t *frame_len; int nframes;
    long long *dst_off;                          // [nframes] workspace: each frame's place
};
hipError_t launch_gather_offsets(hipStream_t st, const GatherFramesArgs &a);
hipError_t launch_gather_frames(hipStream_t st, const GatherFramesArgs &a);

}  // namespace fhip
