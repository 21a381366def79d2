/*
 * flakehip_spans.h -- the span-rows part of libflakehip.so's C ABI (K13): a span of a stream, decoded once, laid into
 * every row of row_len samples, hop apart, that its samples belong to.  K10's re-layout, one to many.  Included by
 * flakehip.h, behind every type it uses; include that, not this.
 */
#ifndef FLAKEHIP_SPANS_H
#define FLAKEHIP_SPANS_H

#ifndef FLAKEHIP_H
#error "include flakehip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A segment of K7's window mode is a run of a SPAN here: its first delivered sample is sample seg_pos[k] of the span,
 * and the span owns the seg_nrows[k] rows from seg_row0[k] on of a fhip_rows_out, row j holding the span's samples
 * [j * hop, j * hop + row_len).  Segment k is delivered when seg_failed[k] < 0, seg_nrows[k] >= 1, seg_row0[k] >= 0,
 * seg_row0[k] + seg_nrows[k] <= nrows, seg_pos[k] >= 0 and 0 <= seg_start[k] < pcm_cap, and then writes, for
 * i in [0, min(seg_samples[k], pcm_cap - seg_start[k])), p = seg_pos[k] + i, every channel c and every j in
 * [0, seg_nrows[k]) with j * hop <= p < j * hop + row_len,
 *   rows[seg_row0[k] + j][c][p - j * hop] = conv(pcm[(seg_start[k] + i) * channels + c])
 * with conv as fhip_rows_out's format has it.  All of it is computed in 64 bits.  Every other segment writes nothing,
 * and nothing else is written: the kernel zeroes nothing -- padding is the caller's (fhip_rows_zero_dev).  Segments of
 * one span must not overlap in span positions, and spans must not share rows.
 */
typedef struct fhip_span_rows {
    const int32_t *seg_row0;      /* [nsegs] the span's first row */
    const int32_t *seg_nrows;     /* [nsegs] the span's rows */
    const int64_t *seg_pos;       /* [nsegs] the span position of the segment's first delivered sample */
    int64_t        hop;           /* 1 .. 2^31 - 1 */
    /* fhip_span_rows_from_segments_dev only (the other entries make their own and do not read these): the tiles of 512
     * samples the launch allots each segment, as a CSR -- DEVICE [nsegs + 1], from 0 to ntiles, not decreasing.  A
     * segment's samples behind its tiles are not delivered, so a segment of up to n samples needs ceil(n / 512). */
    const int32_t *tile_first;
    int32_t        ntiles;
} fhip_span_rows;

/* K13 alone.  All pointers DEVICE pointers, the four of spans included: pcm [pcm_cap][channels] int32, seg_start /
 * seg_samples (int64) and seg_failed (int32) as K7 left them, [nsegs] each.  Asynchronous on the handle's stream, one
 * launch of ntiles workgroups.  The kernel clamps every table index to [0, nsegs), every read into the source and every
 * write into a row of the segment's own whatever the tables hold.  Launch list: "k_span_rows"; timed under that name
 * with fhip_set_profiling.  FHIP_E_INVALID with nothing queued and an empty launch list for null pointers, nsegs < 0,
 * pcm_cap < 0, ntiles < 0, hop < 1 or above 2^31 - 1, nrows < 1, row_len < 1, an unknown format or FHIP_ROWS_I16 on a
 * handle above 16 bits; FHIP_E_UNSUPPORTED under FHIP_PCM_S16 (the source is int32).  nsegs == 0, pcm_cap == 0 or
 * ntiles == 0: nothing is queued. */
FHIP_API int fhip_span_rows_from_segments_dev(fhip_ctx *ctx, const int32_t *pcm, int64_t pcm_cap, int32_t nsegs,
                                              const int64_t *seg_start, const int64_t *seg_samples,
                                              const int32_t *seg_failed, const fhip_span_rows *spans,
                                              const fhip_rows_out *rows);

/* fhip_decode_frames_windows_rows and fhip_decode_frames_windows_rows_held with K13 behind K7 instead of K10: the three
 * tables of spans are HOST memory [nsegs], and the tile CSR is made here, from what a segment's frames can hold at
 * most (its frames times the handle's block_size) and what it was told to take.  Everything else -- in / segs / win,
 * the held source, rows, out, the records, summary, nsamples and per-segment outputs, the single synchronisation,
 * FHIP_OK / FHIP_E_VERIFY -- is theirs.  The launch lists are theirs with "k_span_rows" at the end in "k_window_rows"'
 * place.  FHIP_E_INVALID with nothing queued and an empty launch list for what they refuse, for null span tables and
 * for hop < 1 or above 2^31 - 1; FHIP_E_UNSUPPORTED under FHIP_PCM_S16. */
FHIP_API int fhip_decode_frames_windows_spans(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                              const fhip_decode_windows *win, const fhip_span_rows *spans,
                                              const fhip_rows_out *rows, const fhip_decode_out *out);
FHIP_API int fhip_decode_frames_windows_spans_held(fhip_ctx *ctx, const uint8_t *src_dev, int64_t src_bytes,
                                                   const int64_t *frame_src, const int32_t *frame_len, int32_t nframes,
                                                   const fhip_decode_segments *segs, const fhip_decode_windows *win,
                                                   const fhip_span_rows *spans, const fhip_rows_out *rows,
                                                   const fhip_decode_out *out);

#ifdef __cplusplus
}
#endif
#endif /* FLAKEHIP_SPANS_H */
