/*
 * flakehip_rows_in.h -- the encode-rows part of libflakehip.so's C ABI (K12): a padded planar batch in device memory
 * converted into channel-interleaved int32 PCM, K10's inverse.  Included by flakehip.h, behind every type it uses;
 * include that, not this.
 */
#ifndef FLAKEHIP_ROWS_IN_H
#define FLAKEHIP_ROWS_IN_H

#ifndef FLAKEHIP_H
#error "include flakehip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The source: rows[nrows][channels][row_len] in DEVICE memory, an element being what FHIP_ROWS_* names.  Element e
 * becomes sample x, with b the handle's bits_per_sample:
 *   FHIP_ROWS_I32   x = e                                         the range is the caller's contract, as for every int32 entry
 *   FHIP_ROWS_I16   x = e, sign-extended                          handles of bits_per_sample <= 16 only
 *   FHIP_ROWS_F32   x = clamp(rne(e * 2^(b-1)), -2^(b-1), 2^(b-1) - 1)
 *                   rne rounds to nearest, ties to even; the product is exact (a power of two); NaN gives 0 and the
 *                   infinities clamp; at b = 32 every e * 2^31 >= 2^31 gives INT32_MAX.  The exact inverse of
 *                   fhip_rows_out's FHIP_ROWS_F32 for every sample of up to 24 bits: rows -> FLAC -> rows is the identity.
 */
typedef struct fhip_rows_in {
    const void *rows;             /* DEVICE [nrows][channels][row_len] elements of the format */
    int32_t nrows;                /* >= 1 */
    int32_t format;               /* FHIP_ROWS_* */
    int64_t row_len;              /* >= 1 */
} fhip_rows_in;

/* count samples per channel (>= 1) from column col of row `row` go to sample dst of the destination.  A table is HOST
 * memory, sorted by dst, and tiles [0, total) of the destination exactly (total = the sum of the counts). */
typedef struct fhip_row_piece {
    int32_t row;                  /* 0 .. nrows - 1 */
    int32_t count;                /* samples per channel, >= 1 */
    int64_t col;                  /* first column: col >= 0, col + count <= row_len */
    int64_t dst;                  /* first sample (per channel) in the destination */
} fhip_row_piece;                 /* 24 bytes */

/* K12 alone: dst is DEVICE memory [dst_cap][channels] int32, rows->rows DEVICE memory, pieces a HOST table that is
 * copied before the call returns.  Asynchronous on the handle's stream.  The table is checked on the host before
 * anything is queued -- counts >= 1, sorted by dst and tiling [0, total) with no gap and no overlap, 0 <= row < nrows,
 * col >= 0, col + count <= row_len, total <= dst_cap -- and a table that fails is FHIP_E_INVALID with nothing queued and
 * an empty launch list, as are null pointers, negative counts, nrows < 1, row_len < 1, an unknown format and
 * FHIP_ROWS_I16 on a handle above 16 bits.  FHIP_E_UNSUPPORTED under FHIP_PCM_S16: the destination is int32.  The
 * kernel clamps every table index, read and write regardless (K7's rule).  npieces == 0: nothing is queued.  Launch
 * list: "k_rows_to_pcm"; timed under that name with fhip_set_profiling.  A lane owns four destination samples of every
 * channel; where they lie in one piece and a channel's four columns start on a 16-byte boundary (8 bytes for int16)
 * they are read with one load, elsewhere element by element; the interleaved values are written with 16-byte stores
 * where dst allows. */
FHIP_API int fhip_pcm_from_rows_dev(fhip_ctx *ctx, int32_t *dst, int64_t dst_cap, const fhip_rows_in *rows,
                                    const fhip_row_piece *pieces, int npieces);

/* The optional first step of a packed encode, in place of fhip_frames_packed_upload / _upload_ragged /
 * fhip_frames_packed_gather: the handle's own PCM staging is filled from rows through a piece table.  It is
 * fhip_frames_packed_gather with K12 in K9's place: b->nframes, b->block_size and block_sizes (non-null: the ragged
 * form, a HOST table [b->nframes]) are what they are there, with the same checks and the same restrictions on a handle
 * with allow_vbs; the pieces must cover exactly the batch's samples; b->pcm is a TOKEN, non-null and never
 * dereferenced, and the steps that follow -- fhip_frames_packed_begin(_ragged), fhip_md5_update_uploaded(_ragged),
 * fhip_encode_blocks_vbs_packed_numbered / _ragged_numbered, with K5 behind them under fhip_set_verify -- take a batch
 * with the same pcm as they take an upload: they read the converted samples.  Returns when the conversion is done.
 * Refusals as fhip_pcm_from_rows_dev's, with the staging (max_frames * block_size samples) as the capacity. */
FHIP_API int fhip_frames_packed_from_rows(fhip_ctx *ctx, const fhip_batch *b, const int32_t *block_sizes,
                                          const fhip_rows_in *rows, const fhip_row_piece *pieces, int npieces);

#ifdef __cplusplus
}
#endif
#endif /* FLAKEHIP_ROWS_IN_H */
