/*
 * flakehip_held.h -- the held-streams part of libflakehip.so's C ABI (K11): frames of a store that stays on the device.
 * Included by flakehip.h, behind every type it uses; include that, not this.
 */
#ifndef FLAKEHIP_HELD_H
#define FLAKEHIP_HELD_H

#ifndef FLAKEHIP_H
#error "include flakehip.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* What a frame's header says: flac_header_ok of the handle's format (csrc/flac_header.h), as a record.  All zero where
 * it is not a header of this stream. */
typedef struct fhip_frame_head {
    uint64_t number;              /* the coded frame or sample number */
    int32_t  n;                   /* the block size */
    int32_t  flags;               /* bit 0: ok, bit 1: variable block size, bits 8..15: the header's length in bytes */
} fhip_frame_head;                /* 16 bytes */

/* heads[f] for the frame of frame_bytes[f] bytes at stream + frame_off[f], f in [0, nframes): one lane per frame
 * (k_frame_heads).  All pointers DEVICE pointers; frame_off is int64.  The codes are held against the handle's
 * channels, bits and sample rate and against max_block_size (0: no limit), as fhip_index_frames holds them.  Reads
 * stay inside the frame's range and inside [0, stream_bytes): a frame with frame_bytes[f] <= 0, or whose range leaves
 * the stream, is not ok.  Asynchronous on the handle's stream.  Launch list: "k_frame_heads"; timed under that name.
 * FHIP_E_INVALID with nothing queued and an empty launch list for null pointers and negative counts.  nframes == 0:
 * nothing is queued. */
FHIP_API int fhip_frame_heads_dev(fhip_ctx *ctx, const uint8_t *stream, int64_t stream_bytes, const int64_t *frame_off,
                                  const int32_t *frame_bytes, int32_t nframes, int32_t max_block_size,
                                  fhip_frame_head *heads);

/* Frames of src copied back to back into dst: frame f, frame_len[f] bytes at src + frame_src[f], lands at the sum of
 * the accepted lengths before it (k_gather_offsets, one workgroup, then k_gather_frames, a wave per frame).  A frame
 * is accepted when frame_len[f] >= 1, its range lies inside [0, src_bytes) and its place fits dst_cap; then
 * dst_frame_bytes[f] = frame_len[f].  Any other frame gets dst_frame_bytes[f] = 0 and copies nothing (K7 names it
 * LENGTH).  All pointers DEVICE pointers, at any address modulo 16; frame_src is int64.  Nothing outside
 * [0, src_bytes) is read and nothing outside an accepted frame's own range of [0, dst_cap) is written.  dst and
 * dst_frame_bytes are what fhip_decode_frames_windows_dev takes as stream and frame_bytes.  Asynchronous on the
 * handle's stream.  Launch list: "k_gather_offsets", "k_gather_frames"; timed under those names.  FHIP_E_INVALID with
 * nothing queued and an empty launch list for null pointers, negative counts and nframes above the handle's
 * max_frames.  nframes == 0: nothing is queued. */
FHIP_API int fhip_gather_frames_dev(fhip_ctx *ctx, uint8_t *dst, int64_t dst_cap, int32_t *dst_frame_bytes,
                                    const uint8_t *src, int64_t src_bytes, const int64_t *frame_src,
                                    const int32_t *frame_len, int32_t nframes);

/* fhip_decode_frames_windows and fhip_decode_frames_windows_rows with the stream taken from DEVICE memory: frame f is
 * the frame_len[f] bytes at src_dev + frame_src[f] (HOST tables [nframes], frame_src int64).  The two tables are
 * uploaded -- 12 bytes a frame -- and the gather above lays the frames into the handle's staging, where K7 reads them
 * as it reads an uploaded stream; no stream byte crosses the link.  segs, win, seg_row, seg_col, rows and out, the
 * records, summary, nsamples, per-segment outputs, FHIP_OK / FHIP_E_VERIFY and the single synchronisation are the host
 * forms'.  The launch list is "k_gather_offsets", "k_gather_frames" followed by the host form's.  FHIP_E_INVALID with
 * nothing queued and an empty launch list for what the host forms refuse, for null src_dev or tables, a negative
 * src_bytes or frame_len, nframes above max_frames and a frame range outside [0, src_bytes).  Under FHIP_PCM_S16 as the
 * host forms (rows: FHIP_E_UNSUPPORTED). */
FHIP_API int fhip_decode_frames_windows_held(fhip_ctx *ctx, const uint8_t *src_dev, int64_t src_bytes,
                                             const int64_t *frame_src, const int32_t *frame_len, int32_t nframes,
                                             const fhip_decode_segments *segs, const fhip_decode_windows *win,
                                             const fhip_decode_out *out);
FHIP_API int fhip_decode_frames_windows_rows_held(fhip_ctx *ctx, const uint8_t *src_dev, int64_t src_bytes,
                                                  const int64_t *frame_src, const int32_t *frame_len, int32_t nframes,
                                                  const fhip_decode_segments *segs, const fhip_decode_windows *win,
                                                  const int32_t *seg_row, const int64_t *seg_col,
                                                  const fhip_rows_out *rows, const fhip_decode_out *out);

/* Bytes appended to a store on the device and indexed where they lie: the host bytes [0, nbytes) are uploaded to
 * store + base, K8 runs on that copy (fhip_index_frames' ranges and answers), k_frame_offsets turns its answers into
 * every frame's offset in the store and k_frame_heads reads every frame's header.  frame_bytes and heads (HOST,
 * [frame_cap]) receive the frames found, back to back in range order; range_frames / range_consumed / range_variable
 * (HOST, [nranges]) are fhip_index_frames'.  One synchronisation, a second only beyond 65536 frames, as there.  The
 * launch list is fhip_index_frames_dev's followed by "k_frame_offsets", "k_frame_heads".  FHIP_E_INVALID with nothing
 * queued and an empty launch list for what fhip_index_frames refuses and for bytes that do not fit
 * [base, store_bytes). */
typedef struct fhip_hold_in {
    uint8_t       *store;         /* DEVICE */
    int64_t        store_bytes;   /* its capacity */
    int64_t        base;          /* where the bytes go */
    const uint8_t *bytes;         /* HOST */
    int64_t        nbytes;        /* < 2^31 */
    const int64_t *range_first;   /* HOST [nranges + 1], from 0 to nbytes */
    int32_t        nranges;
    int32_t        max_block_size;
    int32_t        frame_cap;
} fhip_hold_in;
typedef struct fhip_hold_out {
    int32_t *frame_bytes;
    fhip_frame_head *heads;
    int32_t *range_frames;
    int64_t *range_consumed;
    int32_t *range_variable;
} fhip_hold_out;
FHIP_API int fhip_hold_frames(fhip_ctx *ctx, const fhip_hold_in *in, const fhip_hold_out *out);

#ifdef __cplusplus
}
#endif
#endif /* FLAKEHIP_HELD_H */
