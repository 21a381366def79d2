/*
 * flakehip.h -- C ABI of the MI355X (gfx950) prediction/entropy layer.
 *
 * This is the drop-in boundary: the internal seam of libflake that the HIP
 * layer replaces is
 *
 *     int encode_residual(FlacEncodeContext *ctx, int ch)      optimize.h:27
 *                                                              optimize.c:124-276
 * together with its feeder stages in encode_frame() (encode.c:932-942:
 * copy_samples, channel_decorrelation, remove_wasted_bits) and the residual
 * section of output_subframes() (encode.c:766-798 + bitio.h:120-141) --
 * batched over many independent frames.  Everything here is plain C: no HIP,
 * no C++ and no torch types cross the boundary.  Pointers documented as
 * "device" are hipMalloc'd addresses (e.g. a torch tensor's data_ptr()).
 *
 * Error convention follows libflake (negative int on failure, encode.c:925-992)
 * with distinct codes; nothing aborts or throws across the ABI.
 *
 * File:line citations are relative to the reference tree (/root/reference).
 */
#ifndef FLAKEHIP_H
#define FLAKEHIP_H

#include <stdint.h>

#if defined(__GNUC__)
#define FHIP_API __attribute__((visibility("default")))
#else
#define FHIP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FHIP_MAX_ORDER   32     /* MAX_LPC_ORDER, lpc.h:25 */
#define FHIP_MAX_PARTS   256    /* MAX_PARTITIONS, rice.h:34-35 */
#define FHIP_MAX_CH      8      /* FLAC_MAX_CH, encode.h:33 */
#define FHIP_MAX_LAGS    (FHIP_MAX_ORDER + 1)

/* largest block (the reference's limit, encode.h:35); blocks above 16384 take
 * streaming variants of K0 and K3 (correct, not tuned) */
#define FHIP_MAX_BLOCK   65535    /* FLAC's and libflake's limit (encode.c:288) */

enum {
    FHIP_OK            =  0,
    FHIP_E_GENERIC     = -1,    /* libflake's only code */
    FHIP_E_HIP         = -2,    /* a HIP runtime call failed; see fhip_last_error() */
    FHIP_E_UNSUPPORTED = -3,    /* valid libflake parameters this layer does not cover */
    FHIP_E_INVALID     = -4,    /* parameters flake_validate_params() would reject */
    FHIP_E_NOMEM       = -5,
    FHIP_E_VERIFY      = -6     /* the stream does not decode to the input (fhip_set_verify) */
};

/* subframe types (encode.h:37-40) and channel modes (encode.h:42-46) */
enum { FHIP_SUB_CONSTANT = 0, FHIP_SUB_VERBATIM = 1, FHIP_SUB_FIXED = 8, FHIP_SUB_LPC = 32 };
enum { FHIP_CH_NOT_STEREO = 0, FHIP_CH_LEFT_RIGHT = 1, FHIP_CH_LEFT_SIDE = 8,
       FHIP_CH_RIGHT_SIDE = 9, FHIP_CH_MID_SIDE = 10 };

/*
 * The fields of FlakeContext / FlakeEncodeParams (flake.h:59-197) that the
 * path reads, with the same names and value ranges, plus lpc_precision
 * (FlacEncodeContext.lpc_precision, always 15: encode.c:443).
 */
typedef struct fhip_params {
    int channels;                /* 1..8 */
    int sample_rate;
    int bits_per_sample;         /* 4..32 */
    int block_size;              /* params.block_size: the largest block */
    int order_method;            /* FLAKE_ORDER_METHOD_* 0..6, flake.h:38-46 */
    int stereo_method;           /* 0 independent, 1 estimate, flake.h:48-51 */
    int prediction_type;         /* 0 none, 1 fixed, 2 levinson, flake.h:53-57 */
    int min_prediction_order;
    int max_prediction_order;
    int min_partition_order;
    int max_partition_order;
    int variable_block_size;
    int allow_vbs;
    int lpc_precision;
} fhip_params;

/*
 * What encode_residual() leaves in FlacSubframe (encode.h:52-63) and its
 * RiceContext (rice.h:41-46), one record per (frame, channel).
 */
typedef struct fhip_subframe_info {
    int32_t  type;               /* FHIP_SUB_* */
    int32_t  type_code;
    int32_t  order;
    int32_t  shift;
    int32_t  obits;
    int32_t  wasted;             /* FlacSubframe.wasted_bits */
    int32_t  rice_method;        /* RiceContext.method: 0 RICE, 1 RICE2 */
    int32_t  porder;             /* RiceContext.porder */
    uint32_t est_bits;           /* return value of encode_residual() */
    int32_t  ch_mode;            /* FlacFrame.ch_mode, replicated per channel */
    int32_t  rice_nbits;         /* exact bit length of the residual section as
                                    output_residual() writes it; 0 when the
                                    subframe has none; -1 when it does not fit
                                    the caller's slot (nothing written) */
    int32_t  reserved;
    int32_t  coefs[FHIP_MAX_ORDER];
    int32_t  rparams[FHIP_MAX_PARTS];   /* RiceContext.params[0 .. 2^porder) */
    int32_t  warmup[FHIP_MAX_ORDER];    /* residual[0 .. order): the warm-up samples the
                                           subframe header carries (encode.c:834-837,
                                           :851-854); [0] is the value of a CONSTANT
                                           subframe (encode.c:800-807) */
} fhip_subframe_info;

typedef struct fhip_ctx fhip_ctx;

/* ---- lifetime ------------------------------------------------------- */

/* Number of HIP devices, or a negative code. */
FHIP_API int fhip_device_count(void);

/*
 * Create a handle bound to one device.  Plays the role of the buffers
 * flake_encode_init() allocates (encode.c:378-472): device workspaces for
 * max_frames frames of p->block_size samples per channel, so that no call
 * below allocates.  Returns FHIP_E_INVALID where flake_validate_params()
 * (encode.c:268-373) returns -1.
 */
FHIP_API int fhip_create(fhip_ctx **out, int device, const fhip_params *p, int max_frames);
FHIP_API void fhip_destroy(fhip_ctx *ctx);                       /* flake_encode_close, encode.c:1010 */

/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL
 * returns to the handle's own stream.
 * The contract (tests/test_gpu_stream_order.py): every *_dev entry is ordered on the current stream on both
 * sides -- it sees what the caller queued there before the call, and what the caller queues there afterwards
 * sees its results -- with no host synchronisation needed around it.  Its inputs may be rewritten by later work
 * on that stream.  Whatever the entry runs on streams of the handle's own is joined into the current stream
 * before the entry returns.  Switching streams only swaps a pointer: it does NOT order the new stream after the
 * old one; the caller does that (an event, or torch's S2.wait_stream(S1)) before the first call on the new stream.
 * fhip_prepare_ahead is the one exception and says so below. */
FHIP_API int fhip_set_stream(fhip_ctx *ctx, void *hip_stream);
FHIP_API int fhip_sync(fhip_ctx *ctx);

/*
 * The handle's PCM format: the width of the samples every `pcm` pointer given to it addresses.
 *   FHIP_PCM_S32 (default)  channel-interleaved int32, flake_encode_frame()'s contract (flake.h:229)
 *   FHIP_PCM_S16            channel-interleaved int16_t, each value sign-extended to int32 on the device and
 *                           from there on treated as the int32 contract says (with bits_per_sample < 16 it
 *                           must already lie in that range).  16-bit audio then crosses the link and is read
 *                           by the feeder stage at 2 bytes per sample instead of 4.
 * The structs keep their layout: while FHIP_PCM_S16 is set, fhip_batch.pcm, fhip_verify_in.pcm and the pcm
 * arguments of fhip_prepare_frames carry the ADDRESS of int16_t samples in their `const int32_t *`; host-pointer
 * entries upload 2 bytes per value.  Honoured by fhip_encode_subframes(_dev), fhip_encode_frames_packed and its
 * _upload / _begin / _fetch steps, fhip_prepare_ahead, fhip_prepare_frames and fhip_verify_frames(_dev)
 * (including the run behind fhip_set_verify); every output is byte-identical to that of the widened int32 input.
 * Device pcm must be 16-byte aligned as before.  Variable block size is not covered: under FHIP_PCM_S16
 * fhip_encode_blocks_vbs_dev, fhip_encode_blocks_vbs_packed and fhip_vbs_split return FHIP_E_UNSUPPORTED (the
 * ragged path reads pieces where they lie with 16-byte loads; its alignment rules differ for 2-byte samples).
 * Returns FHIP_E_INVALID for a null handle, an unknown format, or FHIP_PCM_S16 on a handle with
 * bits_per_sample > 16.  A pending fhip_prepare_ahead / fhip_frames_packed_upload hint is dropped.
 */
enum { FHIP_PCM_S32 = 0, FHIP_PCM_S16 = 1 };
FHIP_API int fhip_set_pcm_format(fhip_ctx *ctx, int format);

FHIP_API const char *fhip_strerror(int code);
FHIP_API const char *fhip_last_error(const fhip_ctx *ctx);
FHIP_API const char *fhip_version(void);                          /* flake_get_version, encode.c:1028 */

/* ---- the hot path --------------------------------------------------- */

/*
 * One batch of nframes consecutive blocks, all of block_size samples per
 * channel.  All pointers are DEVICE pointers.  pcm follows
 * flake_encode_frame()'s input contract (flake.h:229, encode.c:541-553):
 * channel-interleaved int32, sign-extended to bits_per_sample.
 * Outputs other than info may be NULL.  Asynchronous on the handle's stream.
 */
typedef struct fhip_batch {
    const int32_t      *pcm;          /* [nframes][block_size][channels]; the address of int16_t samples
                                         while the handle's format is FHIP_PCM_S16 (fhip_set_pcm_format) */
    int                 nframes;
    int                 block_size;
    fhip_subframe_info *info;         /* [nframes*channels] */
    int32_t            *residual;     /* [nframes][channels][block_size] FlacSubframe.residual */
    uint8_t            *rice_bits;    /* [nframes*channels][rice_slot_bytes]: the residual
                                         section of each subframe, MSB-first from bit 0 of
                                         its slot; slot bytes past the section are untouched */
    int64_t             rice_slot_bytes;   /* multiple of 4 */
    /* stage outputs for parity checks; NULL in production */
    int32_t            *samples;      /* [nframes][channels][block_size] FlacSubframe.samples
                                         after decorrelation and wasted-bits removal */
    double             *autoc;        /* [nframes*channels][FHIP_MAX_LAGS] compute_autocorr */
    /* whole frames assembled on the device (optional; needs rice_bits):
     * frame header + CRC-8, subframes, CRC-16 and the verbatim fallback,
     * encode.c:718-764, :800-917, :949-964 */
    uint8_t            *frames;       /* [nframes][frame_stride] */
    int64_t             frame_stride; /* multiple of 4, >= fhip_frame_stride() */
    int32_t            *frame_bytes;  /* [nframes] bytes written per frame */
    uint32_t            first_frame_number;   /* FlacEncodeContext.frame_count of frame 0; frame f
                                                 carries first + f (or first + f*block_size when
                                                 allow_vbs: encode.c:969-975) */
    const uint32_t     *frame_numbers;        /* optional [nframes]: explicit number per frame
                                                 (ragged VBS batches); overrides the rule above */
} fhip_batch;

/* Bytes per frame slot that hold any frame of block_size samples: its verbatim
 * size (encode.c:521-527) plus alignment slack. */
FHIP_API int64_t fhip_frame_stride(const fhip_params *p, int block_size);

FHIP_API int fhip_encode_subframes_dev(fhip_ctx *ctx, const fhip_batch *b);

/* Host batch -> the batch's frames back to back in host memory: what the loop around
 * flake_encode_frame() writes to the file (flake.c:633-637), for nframes blocks at once.
 * b->pcm is host memory; b->frame_bytes (host, [nframes]) receives the size of every frame
 * (encode_frame's return value, encode.c:976); b->frame_numbers / first_frame_number as in
 * fhip_encode_subframes; b->info (host) is optional; the other outputs are ignored.  Frames
 * are assembled, packed (exclusive scan of their sizes + copy) and only then brought over:
 * the transfer is the stream's bytes, not the frames' verbatim-size slots.  *out_bytes = the
 * bytes written to out (<= out_cap, else FHIP_E_INVALID and nothing is written). */
FHIP_API int fhip_encode_frames_packed(fhip_ctx *ctx, const fhip_batch *b, uint8_t *out,
                                       int64_t out_cap, int64_t *out_bytes);
/* The same in two steps, for a caller that runs chunks of a stream through several handles
 * side by side (one host thread each) and only knows where a chunk's frames go once the
 * chunks before it have reported their sizes: _begin uploads, encodes, packs and returns the
 * chunk's byte count (b->frame_bytes filled); _fetch brings the packed frames to `out`. */
FHIP_API int fhip_frames_packed_begin(fhip_ctx *ctx, const fhip_batch *b, int64_t *total_bytes);
FHIP_API int fhip_frames_packed_fetch(fhip_ctx *ctx, uint8_t *out, int64_t out_cap);
/* Optional first step of _begin, for the same caller: only the upload of b->pcm (returns when the copy is
 * done).  A following _begin for the same pcm / nframes / block_size skips its own upload.  Several handles
 * that upload at the same time share the link and finish together; taking turns (each chunk's upload behind
 * the one before it) lets every other phase -- kernels, the download of the packed frames -- run beside the
 * next chunk's upload. */
FHIP_API int fhip_frames_packed_upload(fhip_ctx *ctx, const fhip_batch *b);
/* _fetch without waiting for the copy (it runs on a stream of the handle's own, beside the handle's next
 * upload); `out` is complete once fhip_frames_packed_fetch_wait() has returned.  The handle's next _begin
 * orders itself behind a download still in flight. */
FHIP_API int fhip_frames_packed_fetch_async(fhip_ctx *ctx, uint8_t *out, int64_t out_cap);
FHIP_API int fhip_frames_packed_fetch_wait(fhip_ctx *ctx);

/*
 * Ragged batches: the same steps for blocks of DIFFERENT lengths in one call -- the last blocks of many streams
 * (a stream set's tails), each encoded exactly as a uniform call of its own length encodes it.  block_sizes is a
 * HOST table [b->nframes], every entry in 1 .. params.block_size; b->pcm is the blocks back to back, each at its own
 * length; b->block_size must equal the largest entry; frame_numbers / first_frame_number as above (without a table
 * frame f carries first_frame_number + f).  Every frame is byte for byte the frame fhip_encode_frames_packed
 * produces for that block alone, and b->info / b->frame_bytes likewise.  The generic kernel instances run, with a
 * per-frame length table on the device ("ragged" in fhip_last_launches); device slots keep the stride of
 * params.block_size.  While fhip_set_verify is on, frame f must carry its number and hold exactly block_sizes[f]
 * samples (fhip_verify_frames_ragged).  Both PCM formats are honoured (int16 blocks may start at any 2-byte
 * boundary).  _begin_ragged returns FHIP_E_UNSUPPORTED on a handle with allow_vbs (its ragged batches go through
 * fhip_encode_blocks_vbs_ragged_numbered below), and both entries with params.block_size > 16384 (callers fall back
 * to one uniform call per length); FHIP_E_INVALID for a bad table, with nothing queued.  The fetch steps are
 * fhip_frames_packed_fetch*.  _upload_ragged is the optional first step, as fhip_frames_packed_upload is; on a handle
 * with allow_vbs it takes int32 PCM only (FHIP_E_UNSUPPORTED under FHIP_PCM_S16) and at most max_frames / 8 blocks,
 * and what it brings is encoded by fhip_encode_blocks_vbs_ragged_numbered.
 */
FHIP_API int fhip_frames_packed_upload_ragged(fhip_ctx *ctx, const fhip_batch *b, const int32_t *block_sizes);
FHIP_API int fhip_frames_packed_begin_ragged(fhip_ctx *ctx, const fhip_batch *b, const int32_t *block_sizes,
                                             int64_t *total_bytes);

/* Page-locked host memory for the host-pointer entries above (libflake mallocs its frame buffer,
 * encode.c:453-454; a caller's PCM is whatever it read the file into, flake.c:622-630): copies from
 * and to pageable memory go through the runtime's bounce buffers at ~2/3 of the link's rate.
 *   fhip_host_alloc / _free        a page-locked buffer (NULL when the runtime refuses)
 *   fhip_host_register / _unregister   page-lock a range the caller owns, in place; the range must
 *                                  stay mapped until it is unregistered.  FHIP_E_HIP when refused
 *                                  (the copies then run as before).
 * None of them needs a handle; all are optional. */
FHIP_API void *fhip_host_alloc(size_t bytes);
FHIP_API void fhip_host_free(void *p);
FHIP_API int fhip_host_register(void *p, size_t bytes);
FHIP_API int fhip_host_unregister(void *p);

/* The same for a variable-block-size stream (encode_frame_vbs, vbs.c:85-119, per block):
 * nblocks blocks of block_size samples in host memory -> every block split by split_frame_v1
 * (vbs.c:36-83) on the device, the pieces encoded (one pass of the path per piece length,
 * fhip_encode_blocks_vbs_dev below), the frames packed in stream order and fetched.
 * Frames are numbered by their first sample (encode.c:969-975: allow_vbs), starting at
 * first_frame_number for the first sample of pcm.  block_bytes[b] = bytes of block b's frames
 * (the return value of flake_encode_frame for that block); block_frames[b] (optional) = how many
 * frames it became; *max_frame_bytes = the largest frame (encode.c:967); *next_frame_number =
 * the number the next block's first frame takes.  The handle must have been created with
 * variable_block_size and allow_vbs set and max_frames >= 8 * nblocks. */
FHIP_API int fhip_encode_blocks_vbs_packed(fhip_ctx *ctx, const int32_t *pcm, int nblocks,
                                           int block_size, uint32_t first_frame_number,
                                           uint8_t *out, int64_t out_cap, int32_t *block_bytes,
                                           int32_t *block_frames, int64_t *out_bytes,
                                           int32_t *max_frame_bytes, uint32_t *next_frame_number);

/* The same with the blocks and the stream DEVICE-RESIDENT, and no host synchronisation inside:
 * pcm (device) -> split_frame_v1 per block, the piece tables (a piece is k eighths of its block:
 * eight bins of equal length, counted and scanned on the device), the path once per bin with the
 * pieces encoded where they lie, the frames packed in stream order into out->packed (device).
 * Asynchronous on the handle's stream; the host learns nothing about the split unless it reads
 * the outputs back.  All pointers in fhip_vbs_out are device pointers:
 *   packed        the frames back to back (vbs.c:104-116 for every block, concatenated)
 *   packed_cap    its size in bytes; a stream that does not fit sets totals[3] and frames past
 *                 the end are not written
 *   frame_bytes   optional [8 * nblocks]: size of the stream's i-th frame, i < totals[0]
 *   block_bytes   optional [nblocks]: bytes of block b's frames (flake_encode_frame's return value)
 *   block_frames  optional [nblocks]: frames block b became (1 = left whole, vbs.c:100)
 *   totals        [4] int64: frames, bytes, largest frame (encode.c:967), flags -- bit 0: the stream was cut
 *                 (did not fit packed_cap), bit 1: some frame of the stream was not encoded (frame_bytes <= 0;
 *                 its bytes are missing from packed)
 * pcm must be 16-BYTE ALIGNED (the splitter and the feeder stage read the blocks where they lie with
 * 16-byte loads); a misaligned pointer is refused with FHIP_E_INVALID.
 * Frame numbers as in fhip_encode_blocks_vbs_packed.  The handle: variable_block_size and
 * allow_vbs set, max_frames >= 8 * nblocks.  Such a handle sizes its subframe-indexed workspaces
 * (autoc, coefs 4 KB, shift, fin, K0 records) for 20 frame slots per block -- 2.5 x max_frames frames --
 * in fhip_create, whether or not a variable-block-size batch is ever run on it: create handles that
 * only see uniform batches without variable_block_size. */
typedef struct fhip_vbs_out {
    uint8_t  *packed;
    int64_t   packed_cap;
    int32_t  *frame_bytes;
    int32_t  *block_bytes;
    int32_t  *block_frames;
    int64_t  *totals;
} fhip_vbs_out;
FHIP_API int fhip_encode_blocks_vbs_dev(fhip_ctx *ctx, const int32_t *pcm, int nblocks, int block_size,
                                        uint32_t first_frame_number, const fhip_vbs_out *out);

/*
 * fhip_encode_blocks_vbs_packed for blocks of MANY STREAMS (a stream set at levels 9-12): block b belongs to some
 * stream and its first sample is that stream's sample block_first[b] (HOST table [nblocks]); its frames are numbered
 * block_first[b] + the frame's offset inside the block, wrapping at 32 bits as the single-stream sum does.  Everything
 * else -- split_frame_v1 per block, the bins, the frames packed in batch order -- is that entry's, and the bytes of
 * block b are those it writes for the block at first_frame_number = block_first[b].  block_bytes [nblocks] is
 * required; block_frames and block_max_frame (block b's largest frame: each stream's own encode.c:967) are optional.
 * The call consumes a pending fhip_frames_packed_upload of the same pcm / nblocks / block_size, as
 * fhip_frames_packed_begin does, so that fhip_md5_update_uploaded between the two runs K6 beside the encode kernels.
 * While fhip_set_verify is on, the stream is verified in the block-table mode (fhip_verify_frames_blocks) before the
 * call returns: FHIP_E_VERIFY and fhip_last_verify_failure as for the other entries, nothing copied to `out`.
 * int32 PCM only (FHIP_E_UNSUPPORTED under FHIP_PCM_S16).
 */
FHIP_API int fhip_encode_blocks_vbs_packed_numbered(fhip_ctx *ctx, const int32_t *pcm, int nblocks, int block_size,
                                                    const uint32_t *block_first, uint8_t *out, int64_t out_cap,
                                                    int32_t *block_bytes, int32_t *block_frames,
                                                    int32_t *block_max_frame, int64_t *out_bytes);
/*
 * The same for blocks of DIFFERENT lengths -- the last blocks of many streams at levels 9-12 -- in ONE batch:
 * block_sizes is a HOST table [nblocks], every entry in 1 .. params.block_size, pcm the blocks back to back at their own
 * lengths.  A block split_frame_v1 sees (a multiple of 8, at least 128 samples: encode.c:997-999) is scored and cut on
 * the device, its eighth being its own length / 8; any other block is one frame.  The pieces go to dense tables in stream
 * order on the device (length, offset, window constant, number), their count stays there, and the ragged generic
 * kernels ("ragged" in fhip_last_launches; every order method in-kernel) run once over a grid sized for 8 * nblocks
 * frames -- no bins, no host synchronisation between the split and the pack.
 *   The contract: the bytes and the three per-block records of block b are exactly what the existing entries write for
 *   that block alone -- fhip_encode_blocks_vbs_packed_numbered with one block of that length where the splitter sees it,
 *   fhip_frames_packed_begin under fhip_set_block_numbering(1) with frame_numbers = {block_first[b]} otherwise -- and do
 *   not depend on the block's position or its neighbours in the call.
 * It consumes a pending fhip_frames_packed_upload_ragged of the same pcm / nblocks / block_sizes, so that
 * fhip_md5_update_uploaded_ragged between the two runs K6 beside the encode kernels.  While fhip_set_verify is on, the
 * stream is verified in the ragged block-table mode (fhip_verify_frames_blocks_ragged) before the call returns:
 * FHIP_E_VERIFY with nothing copied to `out`; fhip_last_verify_failure and fhip_last_verify_number as for the entry above.
 * Refused, with nothing launched and the handle still usable: a handle without variable block size, a size of 0 or above
 * params.block_size, 8 * nblocks > max_frames, a null argument (block_frames and block_max_frame are optional):
 * FHIP_E_INVALID; FHIP_PCM_S16 (int32 only, as every variable-block-size entry) and params.block_size > 16384 (the
 * ragged K3's limit: callers fall back to one call per length): FHIP_E_UNSUPPORTED.  An out_cap that is too small:
 * FHIP_E_INVALID after the batch has run, nothing written, as for the entry above.
 */
FHIP_API int fhip_encode_blocks_vbs_ragged_numbered(fhip_ctx *ctx, const int32_t *pcm, int nblocks,
                                                    const int32_t *block_sizes, const uint32_t *block_first,
                                                    uint8_t *out, int64_t out_cap, int32_t *block_bytes,
                                                    int32_t *block_frames, int32_t *block_max_frame, int64_t *out_bytes);
/*
 * Off by default; FHIP_E_UNSUPPORTED on a handle without allow_vbs.  While on, fhip_batch.frame_numbers of
 * fhip_frames_packed_begin (and fhip_encode_frames_packed) are the first-sample numbers of ONE-FRAME BLOCKS OF
 * INDEPENDENT STREAMS: K4 writes whatever the table holds, as before, and verification (fhip_set_verify) holds frame
 * f to frame_numbers[f] in the block-table mode, one frame per block, instead of checking that the numbers run on
 * from frame_numbers[0].  This is the path for the block lengths variable block size does not split: no multiple
 * of 8, or below 128 (encode.c:997-999).
 */
FHIP_API int fhip_set_block_numbering(fhip_ctx *ctx, int on);

/* Optional hint for a caller that streams batch after batch through one handle
 * (flake.c:622-663 calls flake_encode_frame block after block): start the feeder
 * stage of the NEXT batch -- copy_samples + channel_decorrelation +
 * remove_wasted_bits, encode.c:541-694 -- now, on a stream of the handle's own,
 * so that it runs beside the autocorrelation of the batch in flight (K0 is
 * HBM-bound, K1 is not).  Only next->pcm, nframes and block_size are read.
 * Contract: next->pcm (device memory) already holds the samples when this is
 * called -- it is NOT ordered after work queued on the handle's stream -- and
 * stays unchanged until the fhip_encode_subframes_dev() call for the same
 * pcm / nframes / block_size, which must be the next encode call on this handle,
 * has completed.  That call then skips its own feeder stage; its results are
 * identical with or without the hint.  A hint that the next call does not match
 * (or a batch that asks for `samples` / `autoc`) is dropped without effect. */
FHIP_API int fhip_prepare_ahead(fhip_ctx *ctx, const fhip_batch *next);

/* Same with HOST pointers: copies in, runs, copies out, synchronises.  When
 * `frames` is requested, `info` and `rice_bits` may be NULL (the frames are
 * complete; the sections then live only in a device workspace of
 * rice_slot_bytes per subframe, which must still be given). */
FHIP_API int fhip_encode_subframes(fhip_ctx *ctx, const fhip_batch *b_host);

/* ---- stage entry points (HOST pointers, synchronous) ---------------- */
/* Each mirrors one reference function over a batch, for stage-level parity. */

/* lpc_calc_coefs(), lpc.c:224-257, for nsub blocks of n samples.
 * coefs [nsub][32][32], shift [nsub][32] (rows the reference leaves
 * unwritten are zero), opt_order [nsub]; autoc [nsub][33] optional. */
FHIP_API int fhip_lpc_calc_coefs(fhip_ctx *ctx, const int32_t *samples, int nsub, int n,
                        int max_order, int precision, int omethod,
                        int32_t *coefs, int32_t *shift, int32_t *opt_order,
                        double *autoc);

/* encode_residual(), optimize.c:124-276, on prepared samples [nsub][n] with
 * info[s].obits set by the caller; uses the handle's params. */
FHIP_API int fhip_encode_residual(fhip_ctx *ctx, const int32_t *samples, int nsub, int n,
                         fhip_subframe_info *info, int32_t *residual,
                         uint8_t *rice_bits, int64_t rice_slot_bytes);

/* The bits[] table of encode_residual()'s LPC order searches (optimize.c:201-261: 2/4/8-LEVEL,
 * SEARCH, LOG) on prepared samples [nsub][n]: bits[s][order - 1] = the size estimate the
 * reference computes for that order (encode_residual_lpc + calc_rice_params_lpc, optimize.c:207-212,
 * :228-233, :250-255) for every order the handle's method visits, 0xFFFFFFFF for the others and
 * for a constant block.  info[s].obits as for fhip_encode_residual; bits 8..15 of
 * info[s].reserved may carry 1 + m with |x| < 2^m for every sample (what the feeder stage
 * records; 0 = unknown), which lets 16-bit blocks take the packed FIRs.  FHIP_E_UNSUPPORTED where
 * the search runs inside the encode kernel (other block sizes / methods).  bits: [nsub][32]. */
FHIP_API int fhip_order_search_bits(fhip_ctx *ctx, const int32_t *samples, int nsub, int n,
                           const fhip_subframe_info *info, uint32_t *bits);

/* calc_rice_params_lpc() / calc_rice_params_fixed(), rice.c:173-187, plus the
 * residual section of output_residual() (encode.c:766-798) on GIVEN residuals
 * [nsub][n]: fills info[].rice_method/porder/rparams/est_bits/rice_nbits. */
FHIP_API int fhip_calc_rice_params(fhip_ctx *ctx, const int32_t *residual, int nsub, int n,
                                   int pred_order, int lpc, int bps, int pmin, int pmax,
                                   fhip_subframe_info *info, uint8_t *rice_bits,
                                   int64_t rice_slot_bytes);

/* split_frame_v1(), vbs.c:36-83, for nblocks blocks of block_size samples per
 * channel (block_size a multiple of 8, >= 128): frames [nblocks] and
 * sizes [nblocks][8] exactly as the reference computes them. */
FHIP_API int fhip_vbs_split(fhip_ctx *ctx, const int32_t *pcm, int nblocks, int block_size,
                            int32_t *frames, int32_t *sizes);
/* The same for blocks of different lengths back to back (block_sizes: HOST [nblocks], 1 .. params.block_size), as
 * fhip_encode_blocks_vbs_ragged_numbered splits them: a block of a multiple of 8 and at least 128 samples as above
 * with its own eighth, any other one frame of its length (frames[b] = 1, sizes[b] = {n, 0, ...}).  The checks and
 * refusals are that entry's. */
FHIP_API int fhip_vbs_split_ragged(fhip_ctx *ctx, const int32_t *pcm, int nblocks, const int32_t *block_sizes,
                                   int32_t *frames, int32_t *sizes);

/* copy_samples + channel_decorrelation + remove_wasted_bits,
 * encode.c:541-694, for nframes blocks; fills info[].obits/wasted/ch_mode. */
FHIP_API int fhip_prepare_frames(fhip_ctx *ctx, const int32_t *pcm, int nframes, int n,
                        int32_t *samples, fhip_subframe_info *info);

/* ---- verification --------------------------------------------------- */

/*
 * Does every frame of a stream decode, by a FLAC decoder that follows the specification, to the
 * caller's PCM?  The verifier (K5) reads only what is below and the handle's fhip_params -- never
 * what the encoder kept on the side -- and checks, per frame: the header (sync, reserved bits,
 * blocking strategy = allow_vbs, channel assignment, sample-size and sample-rate codes, CRC-8),
 * numbering and coverage (the frames cover [first_sample, first_sample + nsamples) in order, each
 * sample once; a fixed-block stream numbers frames, frame f starting at f * block_size, a
 * variable-block-size one numbers samples), every subframe (CONSTANT, VERBATIM, FIXED 0-4,
 * LPC 1-32, wasted bits, RICE / RICE2, escape partitions), the zero padding, CRC-16 and the length.
 * Samples are restored the way libFLAC does: a 64-bit prediction sum, an arithmetic shift, the
 * sample wrapped to int32.  STREAMINFO's MD5 is not checked.
 */
typedef struct fhip_verify_in {
    const uint8_t *stream;        /* the frames back to back */
    int64_t        stream_bytes;
    const int32_t *frame_bytes;   /* [nframes] size of each frame; frame f starts at the sum of those before it */
    int32_t        nframes;
    const int32_t *pcm;           /* [nsamples][channels] interleaved int32 (flake_encode_frame's contract);
                                     the address of int16_t samples under FHIP_PCM_S16 (fhip_set_pcm_format) */
    int64_t        nsamples;
    int64_t        first_sample;  /* absolute index of pcm[0] in the stream */
} fhip_verify_in;

/* per-frame status: the first failing check in stream order */
enum {
    FHIP_VERIFY_OK = 0,
    FHIP_VERIFY_HEADER = 1,       /* sync, reserved bit, blocking strategy, a code that disagrees with the params */
    FHIP_VERIFY_CRC8 = 2,
    FHIP_VERIFY_NUMBER = 3,       /* frame / sample number, block size or coverage */
    FHIP_VERIFY_SYNTAX = 4,       /* reserved type or coding method, precision 16, negative shift, a partition
                                     order the block cannot take, a read past the frame's end */
    FHIP_VERIFY_SAMPLES = 5,      /* a field decodes to a value other than the input requires */
    FHIP_VERIFY_PADDING = 6,
    FHIP_VERIFY_CRC16 = 7,
    FHIP_VERIFY_LENGTH = 8        /* the frame does not end at its frame_bytes, or runs past the stream */
};

typedef struct fhip_verify_rec {
    int32_t status;               /* FHIP_VERIFY_* */
    int32_t bit;                  /* bit offset within the frame of the first discrepancy; -1 when OK */
    int32_t subframe;             /* the subframe (stream order) it lies in, or -1 */
    int32_t sample;               /* SAMPLES: the sample index within the frame, else -1 */
} fhip_verify_rec;

typedef struct fhip_verify_out {
    fhip_verify_rec *frames;      /* optional [nframes] */
    int64_t         *summary;     /* [4]: frames checked, frames failed, first failing frame (-1: none), its status */
} fhip_verify_out;

/* All pointers DEVICE pointers; asynchronous on the handle's stream, no host synchronisation. */
FHIP_API int fhip_verify_frames_dev(fhip_ctx *ctx, const fhip_verify_in *in, const fhip_verify_out *out);
/* The same with HOST pointers: uploads, runs, synchronises.  FHIP_OK or FHIP_E_VERIFY; on
 * FHIP_E_VERIFY fhip_last_error() names the first failing frame, its status, subframe, sample and bit. */
FHIP_API int fhip_verify_frames(fhip_ctx *ctx, const fhip_verify_in *in, const fhip_verify_out *out);

/*
 * The same two entries for a batch whose frames belong to SEVERAL fixed-block streams (a stream set): frame f must
 * carry exactly frame_numbers[f] ([nframes] uint32: device memory for _dev, host memory for the other, which uploads
 * the table beside the stream, the sizes and the PCM) in its header's UTF-8 field, whatever its neighbours carry;
 * otherwise it fails with FHIP_VERIFY_NUMBER at bit 32.  Its samples are the block_size samples at f * block_size
 * of pcm -- its position in the batch -- and every frame, the last included, must hold exactly params.block_size
 * samples (FHIP_VERIFY_NUMBER at bit 16 otherwise); in->first_sample is ignored.  Everything else -- header codes,
 * CRC-8, subframes, padding, CRC-16, length, the records and the summary -- is as above.  What is NOT checked is
 * which stream a frame belongs to: the table is the caller's statement of that.  frame_numbers == NULL makes them
 * fhip_verify_frames_dev / fhip_verify_frames.  On a handle with allow_vbs (frames numbered by sample, verified in
 * sequence) a table is refused with FHIP_E_UNSUPPORTED and nothing is queued.  On FHIP_E_VERIFY the error text also
 * gives the number the first failing frame was required to carry.
 */
FHIP_API int fhip_verify_frames_numbered_dev(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *frame_numbers,
                                             const fhip_verify_out *out);
FHIP_API int fhip_verify_frames_numbered(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *frame_numbers,
                                         const fhip_verify_out *out);

/*
 * The ragged numbered mode: as fhip_verify_frames_numbered, but frame f must hold exactly block_sizes[f] samples
 * (FHIP_VERIFY_NUMBER at bit 16 otherwise), and they are the samples at frame_src[f] of pcm -- an offset in
 * interleaved values, a multiple of the channel count.  The host form takes a HOST block_sizes (entries in
 * 1 .. params.block_size, their sum in->nsamples: FHIP_E_INVALID otherwise) and places the blocks back to back; the
 * _dev form takes both tables as device memory.  frame_numbers is required.  allow_vbs handles: FHIP_E_UNSUPPORTED.
 */
FHIP_API int fhip_verify_frames_ragged_dev(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *frame_numbers,
                                           const int32_t *block_sizes, const int64_t *frame_src,
                                           const fhip_verify_out *out);
FHIP_API int fhip_verify_frames_ragged(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *frame_numbers,
                                       const int32_t *block_sizes, const fhip_verify_out *out);

/*
 * The block-table mode, for a variable-block-size batch whose blocks belong to SEVERAL streams (allow_vbs handles;
 * FHIP_E_UNSUPPORTED on others): the batch is nblocks blocks of block_size samples (1 .. params.block_size), in->pcm
 * holds them back to back (in->nsamples = nblocks * block_size), each block is one or more frames, and the first
 * sample of block b is sample block_first[b] of its stream ([nblocks] uint32: device memory for _dev, host memory for
 * the other).  The verifier is NOT told how the blocks were split: frame f starts at S_f, the sum of the sizes the
 * headers of the frames before it carry -- what a sequential decoder has counted when it reaches the frame -- so it
 * lies in block S_f / block_size at offset S_f % block_size, and must
 *   carry (uint32)(block_first[blk] + off) in its header                   else FHIP_VERIFY_NUMBER at bit 32
 *   end inside its block (off + n <= block_size), in a block of the table
 *   (blk < nblocks), and, the last frame, at in->nsamples                  else FHIP_VERIFY_NUMBER at bit 16
 * A frame behind one whose header does not parse cannot be placed and fails with FHIP_VERIFY_NUMBER at bit 16 too;
 * the first failing frame the summary names is still the true first.  in->first_sample is ignored.  Everything else
 * is as for fhip_verify_frames.  As with the number table, which stream a block belongs to is the caller's statement.
 */
FHIP_API int fhip_verify_frames_blocks_dev(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *block_first,
                                           int nblocks, int block_size, const fhip_verify_out *out);
FHIP_API int fhip_verify_frames_blocks(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *block_first,
                                       int nblocks, int block_size, const fhip_verify_out *out);
/*
 * The block-table mode with a LENGTH PER BLOCK (the batch of fhip_encode_blocks_vbs_ragged_numbered): block b is
 * block_sizes[b] samples (1 .. params.block_size) and starts at start[b], the sum of the lengths before it.  Frame f
 * starts at S_f as above; it lies in the block b with start[b] <= S_f < start[b + 1] -- a search where the uniform mode
 * divides -- and must carry (uint32)(block_first[b] + S_f - start[b]) (FHIP_VERIFY_NUMBER at bit 32), end inside that
 * block, lie in a block of the table and, the last frame, end at in->nsamples (FHIP_VERIFY_NUMBER at bit 16).  Every
 * other status and the rule for frames behind an unparsable one are the uniform mode's.  The host form takes a HOST
 * block_sizes [nblocks] (an entry out of range: FHIP_E_INVALID); the _dev form takes block_start, the prefix sums
 * themselves as DEVICE int64 [nblocks + 1] (block_start[0] = 0), beside a device block_first.
 */
FHIP_API int fhip_verify_frames_blocks_ragged_dev(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *block_first,
                                                  int nblocks, const int64_t *block_start, const fhip_verify_out *out);
FHIP_API int fhip_verify_frames_blocks_ragged(fhip_ctx *ctx, const fhip_verify_in *in, const uint32_t *block_first,
                                              int nblocks, const int32_t *block_sizes, const fhip_verify_out *out);

/*
 * Verification of the handle's own output, off by default.  While on:
 *   fhip_frames_packed_begin (and fhip_encode_frames_packed) and fhip_encode_blocks_vbs_packed run
 *   the verifier on the device-resident stream and PCM before they return, and return FHIP_E_VERIFY
 *   (copying nothing to `out`) when a frame fails; after a failed _begin, fhip_frames_packed_fetch
 *   still delivers the bytes.  fhip_encode_blocks_vbs_dev sets bit 2 of totals[3] when a frame
 *   fails (no host synchronisation).  The bytes written are the same with verification on or off.
 *   A fixed-block batch with fhip_batch.frame_numbers set is verified against that table, frame by frame (the
 *   semantics of fhip_verify_frames_numbered: the frames may belong to many streams, in any order); without a table
 *   the frames must count up from first_frame_number.  A variable-block-size batch is verified in sequence either way,
 *   unless fhip_set_block_numbering is on (block-table mode, one frame per block); fhip_encode_blocks_vbs_packed_numbered
 *   is verified in the block-table mode.
 *   fhip_frames_packed_begin_ragged is verified with the semantics of fhip_verify_frames_ragged,
 *   fhip_encode_blocks_vbs_ragged_numbered with those of fhip_verify_frames_blocks_ragged.
 */
FHIP_API int fhip_set_verify(fhip_ctx *ctx, int on);
/* What the most recent host-synchronising verification of this handle found (fhip_verify_frames, _numbered, and the
 * encode entries above while fhip_set_verify is on), for callers that act on it rather than print it: summary[4] as
 * in fhip_verify_out, *first = the record of the first failing frame (status OK and -1s when none failed).  Either
 * pointer may be NULL.  Returns 1 when a frame failed, 0 when none did, FHIP_E_INVALID for a null handle. */
FHIP_API int fhip_last_verify_failure(const fhip_ctx *ctx, int64_t *summary, fhip_verify_rec *first);
/* The number that first failing frame was REQUIRED to carry, where a table said so: its entry of a frame number table
 * (the numbered and ragged modes), or block_first[blk] + off in the block-table mode when the frame could be placed
 * (its header parsed, no frame before it was unplaceable, blk < nblocks).  Returns 1 with *number set (number may be
 * NULL), 0 when no frame failed or the number is not known, FHIP_E_INVALID for a null handle.  This is what a caller
 * with many streams needs to name the frame: the frame's index alone does not say where a split block's pieces start. */
FHIP_API int fhip_last_verify_number(const fhip_ctx *ctx, uint32_t *number);

/* ---- decoding ------------------------------------------------------- */

/*
 * FLAC frames back to PCM (K7): a decoder that follows the specification, for a batch of frames whose byte sizes the
 * caller knows (flake_amd_index_frames finds them in a foreign stream, on the CPU).  It accepts what the verifier
 * accepts -- CONSTANT, VERBATIM, FIXED 0-4, LPC 1-32 (precision 1-15, shift 0-31), wasted bits, RICE / RICE2, escape
 * partitions (raw width 0 included), partition orders 0-15 where the block allows them, channel assignments 0-10,
 * 4-32 bits per sample, block sizes 1 .. params.block_size -- and restores samples the way libFLAC does: a 64-bit
 * prediction sum, an arithmetic shift, the sample wrapped to int32 (the side channel of a 32-bit stream is read
 * wrapped to int32 too).  The header codes are held against the handle's channels, bits_per_sample and sample_rate;
 * everything else of fhip_params is unused, so any handle serves, fixed-block or allow_vbs.
 *
 * Frame f's samples start at the sum of the block sizes carried by the headers before it.  A header that fails a
 * check of its own (sync, codes, CRC-8) carries none -- its block size cannot be trusted -- so the frames behind it
 * follow the last good one; a header that is good but misnumbered or too large for pcm_cap keeps its room.  Numbering is the CALL's, not the handle's: with variable_blocks 0 every header carries a frame
 * number, which goes up by 1, and every frame but the last holds the same number of samples; with 1 it carries a
 * sample number, which goes up by the previous frame's size.  Bit 15 of every header must equal variable_blocks.
 * With first_number >= 0 the first frame must carry it; with -1 only continuity is checked.
 *
 * Per frame one fhip_verify_rec with the verifier's status codes (SAMPLES is never returned; `sample` is -1):
 * HEADER, CRC8, NUMBER (numbering, a block larger than params.block_size, or a frame whose samples would not fit
 * pcm_cap: nothing of it is written), SYNTAX (reserved subframe type or coding method, precision code 15, negative
 * shift, a partition order the block cannot take, a read past the frame's end -- a unary run that does not end inside
 * the frame is one), PADDING, CRC16, LENGTH.  A frame that fails leaves unspecified values in its own sample range
 * only; the other frames are decoded as if it were good.  Every stream read stays inside the frame, every write inside
 * [0, pcm_cap): a corrupt stream ends in a status code.  STREAMINFO's MD5 is the caller's to check.
 */
typedef struct fhip_decode_in {
    const uint8_t *stream;        /* the frames back to back */
    int64_t        stream_bytes;
    const int32_t *frame_bytes;   /* [nframes] size of each frame; nframes <= the handle's max_frames */
    int32_t        nframes;
    int32_t        variable_blocks;   /* 0: frames carry frame numbers, 1: sample numbers */
    int64_t        first_number;  /* the number frame 0 must carry; -1: not checked */
} fhip_decode_in;

typedef struct fhip_decode_out {
    int32_t         *pcm;         /* [pcm_cap][channels] interleaved int32; int16_t storage while the handle's format
                                     is FHIP_PCM_S16 (bits_per_sample <= 16, as that format requires) */
    int64_t          pcm_cap;     /* samples per channel */
    fhip_verify_rec *frames;      /* optional [nframes] */
    int64_t         *summary;     /* [4] as fhip_verify_out: frames, frames failed, first failing frame (-1), its status */
    int64_t         *nsamples;    /* [1] samples per channel written: the sizes of the frames whose header, number and
                                     place were good (a frame that fails later still counts: its range is unspecified) */
} fhip_decode_out;

/* All pointers DEVICE pointers; asynchronous on the handle's stream, no host synchronisation.  Starts a launch list
 * ("k_decode_frames", "k_decode", "k_decode_final") and is timed as "k_decode" under fhip_set_profiling.  The restored
 * subframes pass through the handle's sample workspace, so the call must not overlap an encode call of the same
 * handle on another stream; a later encode call is unaffected.  FHIP_E_INVALID with nothing queued and an empty
 * launch list for null pointers, negative counts or nframes > max_frames. */
FHIP_API int fhip_decode_frames_dev(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_out *out);
/* The same with HOST pointers: uploads, runs, downloads, synchronises; it allocates nothing beyond grow-only staging at
 * first use.  Also FHIP_E_INVALID when frame_bytes does not add up to stream_bytes.  FHIP_OK, or FHIP_E_VERIFY when a
 * frame failed: fhip_last_error() names the first failing frame, its status, subframe and bit,
 * fhip_last_verify_failure() returns the same as numbers, and the samples of the good frames are still delivered. */
FHIP_API int fhip_decode_frames(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_out *out);

/*
 * The frames of MANY streams in one call: the batch is cut into nsegs SEGMENTS, runs of consecutive frames that each
 * belong to one stream (CSR: segment s is frames seg_first[s] .. seg_first[s + 1], seg_first[0] = 0,
 * seg_first[nsegs] = nframes; a segment may be empty).  The rules above hold per segment: continuity only against a
 * predecessor in the same segment, the segment's first frame against seg_number[s] (-1: not checked), bit 15 of its
 * headers against seg_variable[s], and on fixed blocks "every frame but the last has one size" inside the segment, whose
 * last frame may be shorter.  in->variable_blocks and in->first_number are not read.  Placement is the batch's: a
 * frame's samples start at the sum of the sizes of all good headers before it, so the segments lie back to back in pcm;
 * pcm_cap, the records, summary and nsamples keep their meaning for the batch as a whole.  Per segment the call
 * leaves seg_start (where its samples begin in pcm), seg_samples (the samples of its frames whose header, number and
 * place were good: nsamples' rule) and seg_failed (the index in the batch of its first frame that failed with any
 * status, -1 if none).  The launch list is "k_decode_frames segments", "k_decode", "k_decode_final",
 * "k_decode_seg_final"; timed as "k_decode".
 */
typedef struct fhip_decode_segments {
    const int32_t *seg_first;     /* [nsegs + 1] */
    int32_t        nsegs;         /* >= 1 */
    const int64_t *seg_number;    /* [nsegs] */
    const int32_t *seg_variable;  /* [nsegs] 0 or 1 */
    int64_t       *seg_start;     /* [nsegs] out */
    int64_t       *seg_samples;   /* [nsegs] out */
    int32_t       *seg_failed;    /* [nsegs] out */
} fhip_decode_segments;

/* The host form's optional hash: segment s is absorbed into states[seg_stream[s]] on the device (K6, from the decoded
 * PCM where it lies, its range being what K7 left in seg_start / seg_samples: no host round trip), segments of one
 * stream in batch order. */
typedef struct fhip_decode_md5 {
    struct fhip_md5_state *states; /* DEVICE memory, nstreams records (declared below) */
    int32_t         nstreams;
    const int32_t  *seg_stream;   /* HOST [nsegs], each 0 .. nstreams - 1 */
} fhip_decode_md5;

/* As fhip_decode_frames_dev; every table and output of segs is DEVICE memory too (the kernels keep every table read and
 * every output inside [0, nsegs) whatever seg_first holds; its values are the caller's).  segs == NULL: exactly
 * fhip_decode_frames_dev.  FHIP_E_INVALID with nothing queued and an empty launch list also for nsegs < 1 or a null
 * table. */
FHIP_API int fhip_decode_frames_segments_dev(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                             const fhip_decode_out *out);
/* As fhip_decode_frames, with HOST tables and outputs in segs: also FHIP_E_INVALID, nothing queued, when seg_first does
 * not start at 0, decreases or does not end at nframes, when a seg_variable is not 0 or 1, a seg_number is below -1 or a
 * seg_stream is outside the states.  segs == NULL (md5 must then be NULL): exactly fhip_decode_frames.  With md5 the
 * hash is queued behind K7 and before the download ("k_md5_ranges<...>" ends the launch list).  FHIP_E_VERIFY when any
 * frame failed; the good segments' samples, all three per-segment outputs and the hashes are still delivered. */
FHIP_API int fhip_decode_frames_segments(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                         const fhip_decode_out *out, const fhip_decode_md5 *md5);

/*
 * WINDOWS: of every segment only a range of its samples is delivered -- seeking, for the frames of many streams at once.
 * seg_skip[s] (>= 0) samples per channel are dropped from the front of segment s and at most seg_take[s] delivered behind
 * them (-1: to the segment's end); both are counted over the sizes of the segment's good headers, as placement is.  A
 * frame whose samples are [o, o + n) of its segment -- o the sum of the sizes carried by the good headers before it in
 * the segment -- delivers [max(o, skip), min(o + n, skip + take)), which may be empty; skip may exceed the first frame
 * or the whole segment.  What the batch delivers lies back to back in pcm, in batch order, and the outputs speak of
 * delivered samples: seg_start[s] is where segment s's begin, seg_samples[s] how many it delivers (of the frames whose
 * header, number and place were good, as before), nsamples the batch's total; pcm_cap and the refusal of a frame that
 * does not fit (NUMBER, bit 16) are about the delivered range, and a frame that delivers nothing always fits.  Every
 * frame of the batch is still decoded and checked in full -- the recurrence needs the whole frame, the CRC-16 covers it
 * -- so records, summary and seg_failed keep their meaning: a frame that fails names itself even where all of its
 * samples are clipped away.  Both PCM formats.  The launch list is "k_decode_frames windows", "k_decode windows",
 * "k_decode_final", "k_decode_seg_final"; timed as "k_decode".
 */
typedef struct fhip_decode_windows {
    const int64_t *seg_skip;      /* [nsegs] >= 0 */
    const int64_t *seg_take;      /* [nsegs] >= 0, or -1 */
} fhip_decode_windows;

/* As fhip_decode_frames_segments_dev, with both tables of win in DEVICE memory (their values are the caller's: a
 * negative skip counts as 0, a negative take as -1).  FHIP_E_INVALID with nothing queued and an empty launch list also
 * for segs == NULL, win == NULL or a null table. */
FHIP_API int fhip_decode_frames_windows_dev(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                            const fhip_decode_windows *win, const fhip_decode_out *out);
/* As fhip_decode_frames_segments without md5 (windows are not hashed), with HOST tables in win: also FHIP_E_INVALID,
 * nothing queued, for a negative seg_skip or a seg_take below -1.  Only the delivered samples are downloaded. */
FHIP_API int fhip_decode_frames_windows(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                        const fhip_decode_windows *win, const fhip_decode_out *out);

/* ---- frame discovery (K8) --------------------------------------------- */

/*
 * Where do the frames of a stream begin?  The answer is the CPU indexer's (flake_amd_index_frames of the host layer),
 * exactly, for every input, good or corrupt.  For one stream s[0 .. bytes):
 *   - position p is a CANDIDATE iff a frame header stands there whose sync, reserved bits, rate, channel and
 *     bits-per-sample codes agree with the handle's format, whose block size is at most max_block_size (where that is
 *     not 0) and 65535, whose UTF-8 number is well formed and whose CRC-8 holds, all inside bytes - p;
 *   - position 0 must be a candidate (else the answer is -1), and its blocking-strategy bit is the stream's;
 *   - from a boundary a (header length len, block size n, number num) the frame ends at the smallest q >= a + len + 2
 *     where the CRC-16 of s[a .. q - 2) is what lies at q - 2 and either q == bytes or q is a candidate with the
 *     stream's strategy bit and the number num + (variable ? n : 1); the next boundary is q;
 *   - the walk stops at the capacity, at q == bytes, or where no such q exists (that frame is not consumed).
 * No limit on a frame's length.  Many streams per call: range r is the bytes range_first[r] .. range_first[r + 1] of
 * `stream`, one stream's frames from its first header on, and the call means exactly
 *   for r in ranges: index range r with capacity frame_cap - (frames found so far)
 * so a range that does not fit is cut as the capacity cuts it, the ranges behind it get 0 frames and 0 consumed, a
 * range that is refused (-1) takes no room and an empty range gives 0 and 0.  Entries of frame_bytes behind the last
 * frame are not written.  All ranges share the handle's channels, bits_per_sample and sample_rate and the call's
 * max_block_size; everything else of fhip_params is unused.
 */
typedef struct fhip_index_in {
    const uint8_t *stream;        /* the ranges' bytes */
    int64_t        stream_bytes;  /* < 2^31 */
    const int64_t *range_first;   /* [nranges + 1] CSR byte offsets: range r is one stream's frames from its first header on */
    int32_t        nranges;       /* >= 1 */
    int32_t        max_block_size;/* STREAMINFO's; 0: not checked (channels, rate, bits per sample are the handle's) */
    int32_t        frame_cap;     /* room in frame_bytes */
} fhip_index_in;

typedef struct fhip_index_out {
    int32_t *frame_bytes;         /* [frame_cap] the sizes of all ranges' frames, back to back in range order */
    int32_t *range_frames;        /* [nranges] frames found; -1: the range does not begin with a header of this format */
    int64_t *range_consumed;      /* [nranges] bytes those frames cover */
    int32_t *range_variable;      /* [nranges] the strategy bit of the range's first header (0 where there is none) */
} fhip_index_out;

/* All pointers DEVICE pointers; asynchronous on the handle's stream, no host synchronisation.  Starts a launch list
 * ("k_index_scan<false>", "k_index_wgscan", "k_index_scan<true>", "k_index_walk", "k_index_ranges", "k_index_emit";
 * the two scans are absent for an empty stream) and is timed per launch under fhip_set_profiling as "k_index_count",
 * "k_index_wgscan", "k_index_scatter", "k_index_walk", "k_index_ranges", "k_index_emit".  range_first is read clamped:
 * every offset into [0, stream_bytes], every range's end to no less than its start, so every stream read stays inside
 * the stream and every header read inside its own range whatever the table holds; every table read and every output
 * stays inside its array.  The working memory (a candidate table of stream_bytes / 5 + nranges + 1 entries of 20
 * bytes -- two headers lie at least five bytes apart, so no candidate is ever dropped -- and a few words per 4 KiB of
 * stream and per range) is the handle's, allocated at first use and grow-only.  FHIP_E_INVALID with nothing queued and
 * an empty launch list for null pointers, nranges < 1, negative counts or stream_bytes >= 2^31. */
FHIP_API int fhip_index_frames_dev(fhip_ctx *ctx, const fhip_index_in *in, const fhip_index_out *out);
/* The same with HOST pointers: uploads, runs, downloads, and waits once (a second time only where the call finds more
 * than 65536 frames: the sizes behind those come in a copy of their own).  Also FHIP_E_INVALID when range_first does
 * not start at 0, decreases or does not end at stream_bytes. */
FHIP_API int fhip_index_frames(fhip_ctx *ctx, const fhip_index_in *in, const fhip_index_out *out);
/* K8's constants, for tests that place frame starts on every residue of a chunk: the bytes per lane and per workgroup
 * of the candidate pass (which takes the CRC-16 prefixes as well), the bytes per lane of the pass that takes the key
 * at a range's end, and x^(-8) modulo the CRC-16 polynomial.  A pure host function; any pointer may be NULL. */
FHIP_API void fhip_index_geometry(int *lane_bytes, int *wg_bytes, int *end_lane_bytes, int *xinv8);

/* ---- MD5 of many streams (K6) ---------------------------------------- */

/*
 * STREAMINFO's MD5 (metadata.c:61-62, md5.c:281-320) is sequential inside a stream and independent across
 * streams: the device carries one running hash per stream, one lane each, and reads the samples where the
 * encoder already has them.  fhip_md5_state is the device twin of the host's running state; callers allocate
 * nstreams of them in DEVICE memory (16-byte aligned, as hipMalloc gives) and treat the contents as opaque.
 */
typedef struct fhip_md5_state {
    uint32_t h[4];               /* the chaining value */
    uint64_t nbytes;             /* message bytes so far */
    uint32_t fill;               /* bytes waiting in tail[], 0..63 */
    uint32_t reserved;
    uint8_t  tail[64];           /* the partial block */
} fhip_md5_state;                /* 96 bytes: records and their tails stay 16-byte aligned */

/* All pointers DEVICE pointers; asynchronous on the handle's stream (fhip_set_stream), no host synchronisation.
 *   _init    states[0 .. nstreams) = the empty message
 *   _update  stream s absorbs, in this order, the blocks seg_block[seg_first[s] .. seg_first[s + 1]) (int32
 *            tables, CSR; seg_first[nstreams + 1] entries): indices of block_size-sample blocks of pcm, i.e. block b
 *            is the block_size * channels interleaved samples at pcm + b * block_size * channels.  pcm follows the
 *            handle's format (fhip_set_pcm_format); channels and bits_per_sample are the handle's.  The message
 *            is the low (bits_per_sample + 7) / 8 bytes of every sample, little-endian (md5.c:281-320).  A stream
 *            with no block keeps its state bit for bit.  Nothing checks the indices against the buffer: they are
 *            the caller's, like every device table.  When a block is a whole number of 64-byte MD5 blocks, pcm is
 *            16-byte aligned and no stream of the call holds a partial block, the kernel builds the message in
 *            registers from 16-byte loads ("fast" in fhip_last_launches); otherwise bytes go through each stream's
 *            tail ("general": correct, not tuned).
 *   _final   digests[s][0 .. 16) from a padded copy of state s; the states stay usable (metadata.c:61-62).
 * FHIP_E_INVALID for null pointers, negative counts, block_size < 1 or > FHIP_MAX_BLOCK; nothing is queued then. */
FHIP_API int fhip_md5_init_dev(fhip_ctx *ctx, fhip_md5_state *states, int nstreams);
FHIP_API int fhip_md5_update_dev(fhip_ctx *ctx, fhip_md5_state *states, int nstreams, const void *pcm,
                                 int block_size, const int32_t *seg_first, const int32_t *seg_block);
FHIP_API int fhip_md5_final_dev(fhip_ctx *ctx, const fhip_md5_state *states, int nstreams, uint8_t *digests);
/* The update over ranges of samples that the DEVICE names: stream s absorbs, in this order, the ranges
 * seg_range[seg_first[s] .. seg_first[s + 1]) (int32 tables, CSR, as _update's); range r is the range_samples[r]
 * samples per channel at sample range_start[r] of pcm (both DEVICE int64: K7's seg_start / seg_samples serve as they
 * are).  A length <= 0 absorbs nothing; a stream with no range keeps its state bit for bit.  Any fill, any length, any
 * start: bytes go through the stream's tail until it is empty, whole 64-byte units (192 at 3 bytes per sample) are
 * then built in registers from loads that need no more than the sample's own alignment, and the rest goes through the
 * tail ("k_md5_ranges<int16_t,2>" in fhip_last_launches).  Nothing checks the ranges against the buffer. */
FHIP_API int fhip_md5_update_ranges_dev(fhip_ctx *ctx, fhip_md5_state *states, int nstreams, const void *pcm,
                                        const int32_t *seg_first, const int32_t *seg_range, const int64_t *range_start,
                                        const int64_t *range_samples);
/* _final with a HOST digests[nstreams][16] (states stay device memory): finalises, copies, synchronises -- once
 * for all streams. */
FHIP_API int fhip_md5_final(fhip_ctx *ctx, const fhip_md5_state *states, int nstreams, uint8_t *digests);
/* Device memory on the current device for callers without a HIP runtime of their own (the host C layer keeps its
 * set's fhip_md5_state array there); NULL when the runtime refuses.  No handle needed. */
FHIP_API void *fhip_device_alloc(size_t bytes);
FHIP_API void fhip_device_free(void *p);
/* The same update for the packed host path, without a second upload: hashes the PCM that this handle's last
 * fhip_frames_packed_upload brought to the device (nblocks blocks of block_size samples; both must match that
 * upload, which must not have been consumed by fhip_frames_packed_begin or displaced by another entry yet:
 * FHIP_E_INVALID otherwise).  seg_first [nstreams + 1] / seg_block [seg_first[nstreams]] are HOST tables, checked
 * against nblocks; states are device memory.  Runs on an internal stream of the handle, beside the kernels of the
 * fhip_frames_packed_begin that follows; it only reads the PCM, and the handle's next upload orders itself behind
 * it.  Updates of the same states through one handle run in call order. */
FHIP_API int fhip_md5_update_uploaded(fhip_ctx *ctx, fhip_md5_state *states, int nstreams, int nblocks,
                                      int block_size, const int32_t *seg_first, const int32_t *seg_block);

/* The same for a ragged upload (fhip_frames_packed_upload_ragged): block b of the tables is the upload's b-th
 * block, block_sizes[b] samples long; nblocks and block_sizes (HOST) must match that upload.  Always the general
 * path ("ragged general" in fhip_last_launches).  Handles with allow_vbs included (the upload that
 * fhip_encode_blocks_vbs_ragged_numbered then consumes). */
FHIP_API int fhip_md5_update_uploaded_ragged(fhip_ctx *ctx, fhip_md5_state *states, int nstreams, int nblocks,
                                             const int32_t *block_sizes, const int32_t *seg_first,
                                             const int32_t *seg_block);

/* ---- gathering spans on the device (K9) ------------------------------ */

/*
 * What joins a decode to an encode without the samples leaving the device: spans of channel-interleaved int32 samples
 * copied from up to two device buffers into one destination.  A piece is count samples per channel (>= 1) found at
 * sample src of source buffer src_buf (0 or 1) and going to sample dst of the destination; the table is HOST memory,
 * sorted by dst, and tiles [0, total) of the destination exactly (total = the sum of the counts).  All three entries
 * below take int32 PCM only: FHIP_E_UNSUPPORTED under FHIP_PCM_S16.
 */
typedef struct fhip_gather_piece {
    int32_t src_buf;              /* 0 or 1 */
    int32_t count;                /* samples per channel, >= 1 */
    int64_t src;                  /* first sample (per channel) in its source */
    int64_t dst;                  /* first sample (per channel) in the destination */
} fhip_gather_piece;              /* 24 bytes */

/* dst, src0, src1: DEVICE memory, with their capacities in samples per channel (a source of capacity 0 may be null
 * and must not be named by a piece).  Asynchronous on the handle's stream; the table is copied before the call
 * returns.  It is checked on the host before anything is queued -- src_buf 0 or 1, counts >= 1, sorted and tiling
 * [0, total) with no gap and no overlap, every source span inside its capacity, total <= dst_cap -- and a table that
 * fails is FHIP_E_INVALID with nothing queued and an empty launch list, as are null pointers and negative counts.
 * The kernel clamps every table index, read and write regardless (K7's rule).  The destination must not overlap a
 * source span that a LATER tile still reads.  npieces == 0: nothing is queued.  Launch list: "k_gather_spans"; timed
 * under that name with fhip_set_profiling.  Where the source and destination addresses of four values agree modulo
 * 16 bytes they move with 16-byte loads and stores, elsewhere with 4-byte loads. */
FHIP_API int fhip_gather_spans_dev(fhip_ctx *ctx, int32_t *dst, int64_t dst_cap, const int32_t *src0, int64_t src0_cap,
                                   const int32_t *src1, int64_t src1_cap, const fhip_gather_piece *pieces, int npieces);

/* The optional first step of a packed encode, in place of fhip_frames_packed_upload / _upload_ragged: the handle's own
 * PCM staging is filled through a piece table from device sources instead of from host memory.  b->nframes,
 * b->block_size and (block_sizes != NULL: the ragged form, a HOST table [b->nframes]) are what they are for the upload
 * entries, with the same checks and the same restrictions on a handle with allow_vbs; the pieces must tile exactly the
 * batch's samples (nframes * block_size, or the sum of block_sizes).  b->pcm is a TOKEN here: non-null and never
 * dereferenced, it only names the batch, and the steps that follow -- fhip_frames_packed_begin(_ragged),
 * fhip_md5_update_uploaded(_ragged), fhip_encode_blocks_vbs_packed_numbered / _ragged_numbered, with K5 behind them
 * under fhip_set_verify -- take a batch with the same pcm as they take an upload.  Returns when the gather is done
 * (as the uploads return when the copy is).  The sources must not be the handle's own staging. */
FHIP_API int fhip_frames_packed_gather(fhip_ctx *ctx, const fhip_batch *b, const int32_t *block_sizes,
                                       const int32_t *src0, int64_t src0_cap, const int32_t *src1, int64_t src1_cap,
                                       const fhip_gather_piece *pieces, int npieces);

/* fhip_decode_frames_segments with the samples LEFT ON THE DEVICE: out->pcm is DEVICE memory of out->pcm_cap samples
 * per channel (int32), K7 writes there and nothing of it is downloaded.  Everything else is the host form's: host
 * stream, tables, records, summary, nsamples and per-segment outputs, the optional K6 hash queued behind K7 (reading
 * out->pcm), one synchronisation, FHIP_OK or FHIP_E_VERIFY. */
FHIP_API int fhip_decode_frames_segments_keep(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                              const fhip_decode_out *out, const fhip_decode_md5 *md5);

/* ---- windows as a padded planar batch on the device (K10) ------------- */

/*
 * What K7's window mode leaves -- the segments' samples back to back, channel-interleaved int32 -- re-laid as
 * rows[nrows][channels][row_len] in DEVICE memory of the caller's, for a consumer on the same device.  Sample x is
 * written as
 *   FHIP_ROWS_I32   x
 *   FHIP_ROWS_I16   (int16_t)x                                    handles of bits_per_sample <= 16 only
 *   FHIP_ROWS_F32   (float)x * 2^-(bits_per_sample - 1)           in [-1, 1): the conversion rounds to nearest even, the
 *                   scaling is exact (exact altogether up to 24 bits)
 * Segment k goes to row seg_row[k] from column seg_col[k] on.  It is delivered when seg_failed[k] < 0,
 * 0 <= seg_row[k] < nrows, 0 <= seg_col[k] < row_len and 0 <= seg_start[k] < pcm_cap, and then writes, for i in
 * [0, min(seg_samples[k], row_len - seg_col[k], pcm_cap - seg_start[k])) and every channel c,
 *   rows[seg_row[k]][c][seg_col[k] + i] = conv(pcm[(seg_start[k] + i) * channels + c]).
 * Every other segment writes nothing, and nothing else is written: the kernel zeroes nothing -- padding is the caller's
 * (fhip_rows_zero_dev).  Segments that share a row must not overlap.
 */
#define FHIP_ROWS_I32 0
#define FHIP_ROWS_I16 1
#define FHIP_ROWS_F32 2

typedef struct fhip_rows_out {
    void   *rows;                 /* DEVICE [nrows][channels][row_len] elements of the format */
    int32_t nrows;                /* >= 1 */
    int32_t format;               /* FHIP_ROWS_* */
    int64_t row_len;              /* >= 1 */
} fhip_rows_out;

/* K10 alone.  All pointers DEVICE pointers: pcm [pcm_cap][channels] int32, seg_start / seg_samples (int64) and
 * seg_failed (int32) as K7 left them, seg_row (int32) and seg_col (int64) the caller's, [nsegs] each.  Asynchronous on
 * the handle's stream.  The kernel clamps every table index to [0, nsegs), every read into the source and every write
 * into its row whatever the tables hold.  Launch list: "k_window_rows"; timed under that name with fhip_set_profiling.
 * FHIP_E_INVALID with nothing queued and an empty launch list for null pointers, nsegs < 0, pcm_cap < 0, nrows < 1,
 * row_len < 1, an unknown format or FHIP_ROWS_I16 on a handle above 16 bits; FHIP_E_UNSUPPORTED under FHIP_PCM_S16
 * (the source is int32).  nsegs == 0 or pcm_cap == 0: nothing is queued. */
FHIP_API int fhip_rows_from_segments_dev(fhip_ctx *ctx, const int32_t *pcm, int64_t pcm_cap, int32_t nsegs,
                                         const int64_t *seg_start, const int64_t *seg_samples, const int32_t *seg_failed,
                                         const int32_t *seg_row, const int64_t *seg_col, const fhip_rows_out *rows);
/* Zero bits -- zero in all three formats -- into rows first_row .. first_row + count of rows, on the handle's stream
 * (a memset, no kernel: the launch list is left empty).  FHIP_E_INVALID for what the entry above refuses of rows, for a
 * negative first_row or count, or a range that ends behind nrows.  count == 0: nothing is queued. */
FHIP_API int fhip_rows_zero_dev(fhip_ctx *ctx, const fhip_rows_out *rows, int32_t first_row, int32_t count);
/* fhip_decode_frames_windows with the samples delivered as rows ON THE DEVICE: host in / segs / win as there, host
 * tables seg_row (int32) and seg_col (int64) [nsegs], rows->rows DEVICE memory.  K7's window mode decodes into the
 * handle's own staging and K10 runs behind it on the same stream, reading seg_start / seg_samples / seg_failed where K7
 * left them: no host round trip in between and no sample downloaded.  Records, summary, nsamples and the per-segment
 * outputs come back as from the host form, with one synchronisation, after which the rows are written.  out->pcm is
 * not read; out->pcm_cap bounds the staging as it does there.  The launch list is the window list with "k_window_rows"
 * at its end.  FHIP_OK or FHIP_E_VERIFY as the host form; FHIP_E_INVALID also for what fhip_rows_from_segments_dev
 * refuses of rows and for null tables; FHIP_E_UNSUPPORTED under FHIP_PCM_S16. */
FHIP_API int fhip_decode_frames_windows_rows(fhip_ctx *ctx, const fhip_decode_in *in, const fhip_decode_segments *segs,
                                             const fhip_decode_windows *win, const int32_t *seg_row,
                                             const int64_t *seg_col, const fhip_rows_out *rows,
                                             const fhip_decode_out *out);

/* ---- held streams: frames of a store that stays on the device (K11) --- */

/* fhip_frame_heads_dev, fhip_gather_frames_dev, fhip_decode_frames_windows_held, fhip_decode_frames_windows_rows_held and
 * fhip_hold_frames: declared in flakehip_held.h, which is part of this interface and needs nothing but this file. */
#ifdef __cplusplus
}
#endif
#include "flakehip_held.h"
/* ---- encode rows: a planar device batch into interleaved PCM (K12) ---- */
/* fhip_pcm_from_rows_dev and fhip_frames_packed_from_rows, with fhip_rows_in and fhip_row_piece: declared in
 * flakehip_rows_in.h, which is part of this interface and needs nothing but this file. */
#include "flakehip_rows_in.h"
/* ---- span rows: a span decoded once into every hop-spaced row (K13) --- */
/* fhip_span_rows_from_segments_dev, fhip_decode_frames_windows_spans and fhip_decode_frames_windows_spans_held, with
 * fhip_span_rows: declared in flakehip_spans.h, which is part of this interface and needs nothing but this file. */
#include "flakehip_spans.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement ---------------------------------------------------- */

/* With profiling on, every kernel launch of the hot path is bracketed by
 * hipEvents on the launch stream. */
FHIP_API int fhip_set_profiling(fhip_ctx *ctx, int on);
/* After fhip_sync(): accumulated milliseconds and launch counts per kernel
 * since the last reset; returns the number of kernels (<= cap). */
FHIP_API int fhip_get_kernel_times(fhip_ctx *ctx, const char **names, double *ms, int *launches,
                          int cap, int reset);
/* The kernel instances the handle's most recent call queued, in launch order, one per launch,
 * spelled as templates (e.g. "k_encode_pow2<16,256,0>"), followed by the switches that change the
 * path without being template arguments, separated by spaces: "split=1" / "split=2" (K1's lags over
 * one or two workgroups per tile), "tail" (K2 runs inside K1), "fused" (K1 applies K0's decisions),
 * "narrow" (16-bit sample rows).  The calls that start a new list are the encode entries
 * (fhip_encode_subframes*, fhip_frames_packed_begin / fhip_encode_frames_packed, the VBS entries)
 * and fhip_prepare_ahead, the fhip_md5_* entries, fhip_decode_frames(_dev), fhip_decode_frames_segments(_dev, _keep), fhip_decode_frames_windows(_dev, _rows),
 * fhip_rows_from_segments_dev, fhip_rows_zero_dev (which leaves it empty),
 * fhip_index_frames(_dev), fhip_gather_spans_dev, fhip_frames_packed_gather, fhip_frame_heads_dev, fhip_gather_frames_dev,
 * fhip_decode_frames_windows_held, fhip_decode_frames_windows_rows_held, fhip_hold_frames, fhip_pcm_from_rows_dev,
 * fhip_frames_packed_from_rows, fhip_span_rows_from_segments_dev and fhip_decode_frames_windows_spans(_held).  A host-side record: it adds no device work.  (One exception:
 * "k_md5_streams<int16_t,2> fast" / "... general" name a choice that is made on the device when the block shape
 * allows the fast path; asking for the list then waits for that launch.)  names[0 .. cap) receive
 * strings owned by the handle, valid until its next such call; returns the number of launches. */
FHIP_API int fhip_last_launches(fhip_ctx *ctx, const char **names, int cap);
/* The tile length of K1's wave-typed kernel for a uniform batch of nsub subframes of n samples at this maximum
 * prediction order: 256 (positions handed from the staging waves to the walking ones per workgroup barrier; the
 * long-tile form, n a multiple of 256), 128 (the original form), or 0 where K1 is not the wave-typed kernel at all.
 * The launch log spells both forms "k_autocorr_wt<...>"; this tells them apart.  A pure host function: no handle,
 * no device work.  It answers for the launches that read prepared samples (every launch of a default build); the
 * fused-prepare instances (FHIP_FUSE in the environment, an experiment that is off by default) keep the 128 form and
 * size their batch from a hint of their own, so for them the answer may name a form that did not run.
 * It honours FHIP_WT_TILE=128, the measurement switch that keeps the 128 form, which the
 * launches read each time as well. */
FHIP_API int fhip_autocorr_tile(int nsub, int n, int max_order);

#ifdef __cplusplus
}
#endif
#endif /* FLAKEHIP_H */
