/*
 * flake_amd.h -- host-side C layer above the HIP C ABI (flakehip.h).
 *
 * Mirrors libflake's public surface (flake.h:217-234) for the path this
 * project accelerates: the structs below are layout-compatible with
 * FlakeEncodeParams (flake.h:59-161) and FlakeContext (flake.h:163-215), and
 * each function names the libflake function it stands in for.  The host layer
 * owns what libflake keeps on the CPU around encode_residual(): frame/subframe
 * headers, CRC-8/16, the verbatim fallback, the frame counter and MD5.
 *
 * File:line citations are relative to the reference tree (/root/reference).
 */
#ifndef FLAKE_AMD_H
#define FLAKE_AMD_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define FLAKE_AMD_API __attribute__((visibility("default")))
#else
#define FLAKE_AMD_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- libflake-compatible encoder surface ----------------------------- */

/* Layout-compatible with FlakeEncodeParams (flake.h:59-161); same field
 * meaning and ranges. */
typedef struct FlakeAmdEncodeParams {
    int compression;             /* 0..12 */
    int order_method;            /* FLAKE_ORDER_METHOD_* 0..6 */
    int stereo_method;           /* 0 independent, 1 estimate */
    int block_size;
    int padding_size;
    int min_prediction_order;
    int max_prediction_order;
    int prediction_type;         /* 0 none, 1 fixed, 2 levinson */
    int min_partition_order;
    int max_partition_order;
    int variable_block_size;
    int allow_vbs;
} FlakeAmdEncodeParams;

/* Layout-compatible with FlakeContext (flake.h:163-215). */
typedef struct FlakeAmdContext {
    int channels;
    int sample_rate;
    int bits_per_sample;
    unsigned int samples;        /* total stream samples, 0 = unknown */
    FlakeAmdEncodeParams params;
    unsigned char *header;       /* allocated by init, freed by close */
    void *private_ctx;
} FlakeAmdContext;

/* flake.h:241-251 FlakeStreaminfo */
typedef struct FlakeAmdStreaminfo {
    unsigned int min_block_size, max_block_size;
    unsigned int min_frame_size, max_frame_size;
    unsigned int sample_rate, channels, bits_per_sample, samples;
    unsigned char md5sum[16];
} FlakeAmdStreaminfo;

/* flake_set_defaults(), encode.c:158-266: params->compression must be set */
FLAKE_AMD_API int flake_amd_set_defaults(FlakeAmdEncodeParams *params);
/* flake_validate_params(), encode.c:268-373: -1 error, 0 ok, 1 ok but non-Subset */
FLAKE_AMD_API int flake_amd_validate_params(const FlakeAmdContext *s);
/* flake_encode_init(), encode.c:378-472: returns the header length (bytes in
 * s->header) or a negative code.  The HIP device is FLAKE_AMD_DEVICE (default
 * 0); up to FLAKE_AMD_BATCH (default 1024) blocks are encoded per GPU batch.
 * FLAKE_AMD_LOOKAHEAD=N (with FlakeContext.samples set) makes the one-block
 * flake_amd_encode_frame() queue N blocks per GPU batch: it returns 0 while it
 * queues and all queued frames at once when it flushes (see flake_host.c).
 * FLAKE_AMD_MD5=0 skips the stream MD5 (STREAMINFO then carries the all-zero
 * "not computed" signature); FLAKE_AMD_HOST_ASSEMBLY=1 / FLAKE_AMD_HOST_VBS=1 move
 * frame assembly / block splitting back to the CPU (for comparison);
 * FLAKE_AMD_TRACE=1 prints the phase times of every batch on stderr. */
FLAKE_AMD_API int flake_amd_encode_init(FlakeAmdContext *s);
/* flake_get_buffer(), encode.c:474-485: frame buffer of flake_amd_encode_frame */
FLAKE_AMD_API void *flake_amd_get_buffer(const FlakeAmdContext *s);
/* flake_encode_frame(), encode.c:979-1008: one block; bytes written or -1 */
FLAKE_AMD_API int flake_amd_encode_frame(FlakeAmdContext *s, const int *samples, int block_size);
/*
 * Batched form of the same call: nblocks consecutive blocks of block_size
 * samples per channel (interleaved), optionally followed by one shorter last
 * block of tail_size samples (0 = none).  Frames are written back to back
 * into out; frame_sizes (optional, [nblocks + (tail_size > 0)], VBS may write
 * several FLAC frames per block -- their total is recorded per block) and the
 * return value give byte counts.  Negative on error.
 */
FLAKE_AMD_API long long flake_amd_encode_frames(FlakeAmdContext *s, const int *samples,
                                                int nblocks, int block_size, int tail_size,
                                                unsigned char *out, size_t out_size,
                                                int *frame_sizes);
/*
 * The same call for a caller that holds 16-bit (or narrower) audio as channel-interleaved int16_t -- what a 16-bit
 * WAV file holds: the samples cross the link and are read on the device at 2 bytes each instead of being widened
 * to int32 on the CPU first.  Semantics, return values and the stream's bookkeeping (frame counter, min / max frame
 * size, the last-block latch, the MD5 -- hashed straight from the caller's buffer) are those of
 * flake_amd_encode_frames(), and the bytes written are identical to what that call writes for the widened samples;
 * calls of the two widths may be mixed on one stream.  Each value is sign-extended to int32 (with bits_per_sample
 * < 16 it must lie in that range, as the int32 contract says).  Returns -1, with flake_amd_last_error() saying why,
 * when bits_per_sample > 16, when the context uses variable block size (levels 9-12), or under the CPU comparison
 * modes FLAKE_AMD_HOST_ASSEMBLY=1 / FLAKE_AMD_HOST_VBS=1.  flake_amd_pin_buffers() takes the int16 buffer as it
 * is (a byte range).  flake_amd_encode_frame() and its look-ahead queue stay int32.
 */
FLAKE_AMD_API long long flake_amd_encode_frames_s16(FlakeAmdContext *s, const int16_t *samples,
                                                    int nblocks, int block_size, int tail_size,
                                                    unsigned char *out, size_t out_size,
                                                    int *frame_sizes);
/* Page-lock the buffers a caller hands to flake_amd_encode_frames() batch after batch (the loop of
 * flake.c:622-663 reads every block into the same buffer), in place: copies from and to pageable memory run
 * at about two thirds of the link's rate.  Either pointer may be NULL (left as it is); bytes = 0 releases a
 * range.  The ranges must stay mapped until released, replaced or the stream is closed.  Returns 0, or -1
 * when a range was refused (encoding works as before).  The look-ahead queue of flake_amd_encode_frame()
 * and its frame buffer are page-locked by the library itself.  FLAKE_AMD_PIN=0 disables both. */
FLAKE_AMD_API int flake_amd_pin_buffers(FlakeAmdContext *s, const int *samples, size_t sample_bytes,
                                        unsigned char *out, size_t out_bytes);
/* flake_encode_close(), encode.c:1010-1026 */
FLAKE_AMD_API void flake_amd_encode_close(FlakeAmdContext *s);
/* flake_get_streaminfo() / flake_write_streaminfo(), metadata.c:32-84 */
FLAKE_AMD_API int flake_amd_get_streaminfo(const FlakeAmdContext *s, FlakeAmdStreaminfo *si);
FLAKE_AMD_API void flake_amd_write_streaminfo(const FlakeAmdStreaminfo *si, unsigned char *data34);
FLAKE_AMD_API const char *flake_amd_get_version(void);
/* Verification on the device, off by default (not a field: FlakeAmdEncodeParams keeps libflake's layout).
 * While on, every frame an encode call writes is checked to decode, by a FLAC decoder that follows the
 * specification, to the samples it was given (fhip_verify_frames, include/flakehip.h); a batch that fails
 * makes the call return -1 with flake_amd_last_error() naming the frame.  The bytes are the same either way.
 * Call after flake_amd_encode_init(); returns 0, or -1 without a context. */
FLAKE_AMD_API int flake_amd_set_verify(FlakeAmdContext *s, int on);
/* Text of the last error of this context ("" if none). */
FLAKE_AMD_API const char *flake_amd_last_error(const FlakeAmdContext *s);

/* ---- stream sets: many independent streams per batch ------------------ */

/*
 * A set is nstreams streams that share `like`'s channels, sample rate, bits per sample and encoding parameters
 * (validated as flake_amd_encode_init validates them; `like` need not be initialised and is not kept).  The caller
 * hands over blocks of many streams at once and scatters the frames to its files; each stream's frames and
 * STREAMINFO are byte-identical to what a FlakeAmdContext of its own writes for that stream's samples.
 *
 * Each stream's MD5 is carried ON THE DEVICE, one lane per stream, read from the PCM the encoder has already
 * uploaded: the host hashes nothing.  That pays with many streams -- MD5 has no parallelism inside a stream, so the
 * device's time is the length of one stream's share of the batch.  Measured per 4096 blocks of 4096 stereo 16-bit
 * samples: 3.4 ms with 4096 streams and 4.2 ms with 256, against 68 ms for one stream hashed
 * on the host; 52 ms with 16 streams, where FLAKE_AMD_SET_MD5_HOST takes 71 ms.  A lane hashes 85-90 MB/s, one CPU
 * core about 1 GB/s: below about a dozen streams the device hash LOSES to the host and FLAKE_AMD_SET_MD5_HOST is
 * the faster choice; the library does not switch by itself.
 *
 *   FLAKE_AMD_SET_MD5_HOST   hash each stream on the CPU, on the calling thread (the comparison leg)
 *   FLAKE_AMD_SET_MD5_OFF    no MD5: STREAMINFO carries the all-zero "not computed" signature
 *   FLAKE_AMD_SET_VBS        a set with variable block size (`like` at levels 9-12; an error on any other): see below
 *
 * Returns NULL -- flake_amd_set_last_error(NULL) says why -- for invalid parameters, variable block size (levels
 * 9-12) without FLAKE_AMD_SET_VBS, unknown flags, or under the CPU comparison modes FLAKE_AMD_HOST_ASSEMBLY=1 / FLAKE_AMD_HOST_VBS=1.  The
 * device is FLAKE_AMD_DEVICE, the blocks per GPU batch FLAKE_AMD_BATCH (default 1024), as for single streams.
 * Verification is offered for sets through flake_amd_set_enable_verify below (flake_amd_set_verify is the single
 * stream's switch): the verifier holds every frame of a batch to its own stream's frame counter, whichever stream
 * owns it.  Blocks of different sizes share a call through flake_amd_set_encode_ragged.
 *
 * Variable block size (FLAKE_AMD_SET_VBS).  The set then behaves as a context of levels 9-12 does per stream: a block
 * may be written as up to eight frames (frame_sizes[b] is their total, as flake_amd_encode_frames documents), frames
 * are numbered by their stream's sample count, a short block does NOT end its stream (encode.c:993: later blocks of
 * that stream are accepted), STREAMINFO reports min_block_size 16, and samples are int32 only (sample_bytes 2 returns
 * -1).  A block_size that is a multiple of 8 and at least 128 is split on the device
 * (fhip_encode_blocks_vbs_packed_numbered); any other length is one frame per block.  All three MD5 modes and
 * verification work; on a verification failure flake_amd_set_last_verify_failure gives the failing frame's stream
 * and FIRST-SAMPLE number.  flake_amd_set_encode_ragged keeps its argument rules; the short blocks of a call, each
 * of its own length, run as one device batch per FLAKE_AMD_BATCH of them (fhip_encode_blocks_vbs_ragged_numbered:
 * split where the splitter sees them, numbered from their streams' sample counts; FLAKE_AMD_SET_RAGGED=0 keeps one
 * call per distinct length, as do set block sizes above 16384).  The handle is sized for FLAKE_AMD_BATCH * 8 frames, as flake_amd_encode_init sizes it.  Measured per
 * 4096 blocks of 4096 stereo 16-bit samples (tools/set_vbs_bench.py): 5.8 ms at level 10 and 8.0 ms
 * at level 12 over 4096 streams, against 78 ms for one stream with its host MD5.
 */
#define FLAKE_AMD_SET_MD5_HOST 1u
#define FLAKE_AMD_SET_MD5_OFF  2u
#define FLAKE_AMD_SET_VBS      4u
typedef struct FlakeAmdSet FlakeAmdSet;
FLAKE_AMD_API FlakeAmdSet *flake_amd_set_open(const FlakeAmdContext *like, int nstreams, unsigned flags);
/*
 * One batch: nblocks blocks of block_size samples per channel, back to back in `samples` (channel-interleaved
 * int32 with sample_bytes 4, int16_t with 2 -- bits_per_sample <= 16 only); block b belongs to stream
 * stream_of_block[b].  The blocks of one stream appear in stream order; otherwise any interleaving.  `out`
 * receives the frames back to back in batch order, frame_sizes[b] (optional) block b's frame size; the return
 * value is their sum, or -1 (flake_amd_set_last_error).  A block_size below the streams' block size ends the
 * streams it is given for (encode.c:991-992) -- this is how tails are written; tails of equal length may share a
 * call, each stream at most one.  A block for a stream that has ended, a stream index outside the set or a bad
 * argument makes the call return -1 with nothing changed for any stream.
 */
FLAKE_AMD_API long long flake_amd_set_encode(FlakeAmdSet *g, const void *samples, int sample_bytes, int nblocks,
                                             int block_size, const int *stream_of_block, unsigned char *out,
                                             size_t out_size, int *frame_sizes);
/*
 * The same with a length per block: block b is block_sizes[b] samples per channel (1 .. the streams' block size), the
 * blocks back to back in `samples`, each at its own length.  This is how the tails of many streams -- which almost
 * never share a length -- are written in ONE call.  The rules are flake_amd_set_encode's: a block shorter than the
 * streams' block size ends its stream, so each stream has at most one and it is the stream's last block of the call;
 * a stream's blocks appear in stream order; the frames arrive in batch order; an error (a second short block or a
 * block behind a short one for a stream, a stream index outside the set, a size of 0 or above the block size, a bad
 * argument) returns -1 with nothing changed for any stream.  Full-length and short blocks may share a call: the full
 * ones take flake_amd_set_encode's path, the short ones the ragged packed path (fhip_frames_packed_begin_ragged,
 * include/flakehip.h: the generic kernels with a length per frame), each frame byte for byte what a call of its own
 * length writes.  Every MD5 mode, both sample widths and verification (flake_amd_set_enable_verify) work as above.
 *   FLAKE_AMD_SET_RAGGED=0   (environment) the short blocks take one flake_amd_set_encode call per distinct length
 *                            instead -- the comparison leg, and what the entry does by itself where the ragged path
 *                            does not cover the set (block sizes above 16384).
 * Closing S streams with distinct tails takes one call per FLAKE_AMD_BATCH short blocks instead of S calls;
 * tools/set_tail_bench.py times both legs.
 */
FLAKE_AMD_API long long flake_amd_set_encode_ragged(FlakeAmdSet *g, const void *samples, int sample_bytes, int nblocks,
                                                    const int *block_sizes, const int *stream_of_block,
                                                    unsigned char *out, size_t out_size, int *frame_sizes);
/*
 * Encode rows: audio that already lies on the set's device as a padded planar batch -- rows_dev, DEVICE memory
 * [nrows][channels][row_len] of int32, int16 (sets of at most 16 bits) or float32 (format: FLAKE_AMD_ROWS_I32 / _I16 /
 * _F32, below) -- encoded without a sample crossing the link.  The counterpart of flake_amd_decode_set_windows_rows.
 * Row r is the next len_of_row[r] samples (0 .. row_len) of stream stream_of_row[r]; it is cut into len / B whole blocks
 * (B: the streams' block size) and, where len % B != 0, one short block.  An element e becomes the sample
 *   int32, int16   e
 *   float32        clamp(rne(e * 2^(bits_per_sample - 1)), -2^(b-1), 2^(b-1) - 1): round to nearest, ties to even; NaN
 *                  gives 0, infinities clamp -- the exact inverse of FLAKE_AMD_ROWS_F32 on the decode side for every
 *                  sample of up to 24 bits, so rows -> FLAC -> rows is the identity.
 * (K12, fhip_frames_packed_from_rows in include/flakehip_rows_in.h, converts into the handle's own staging.)
 * Contract: for every stream the frames, the STREAMINFO (MD5 included) and the stream's state afterwards are what two
 * host calls on the converted samples give: flake_amd_set_encode on the call's whole blocks, in (row, block) order,
 * followed by flake_amd_set_encode_ragged on its short blocks, in row order.  So the set's own rules decide: a short
 * block ends its stream on a fixed-block set and not on a FLAKE_AMD_SET_VBS set; a stream has at most one short block
 * in a call and may have several rows as long as the resulting block sequence is legal; a row whose length is a
 * multiple of B leaves its stream open, so long audio continues in a later call.  Chunking by FLAKE_AMD_BATCH, seek
 * points, verification, the device MD5 and the VBS levels work as for those calls.
 * out receives all whole blocks' frames in (row, block) order, then the short blocks' frames in row order;
 * row_whole_bytes[r] and row_tail_bytes[r] (both required, [nrows]) say how many bytes of each part are row r's, so
 * that prefix sums place every row.  Returns the total, or -1.  Every argument rule of both parts is checked before
 * anything is encoded: such an error leaves every stream unchanged.  A device failure or an output buffer that is too
 * small behaves as in flake_amd_set_encode; where it strikes the short blocks after the whole blocks were committed,
 * the set refuses further calls.  Refused with -1 and a message: sets opened with FLAKE_AMD_SET_MD5_HOST (no PCM is on
 * the host) and, where a row has a short block, sets whose block size is above 16384 (no ragged path there).  Nothing
 * is pending on the device when the call returns; the caller makes sure the rows are written before it calls.
 */
FLAKE_AMD_API long long flake_amd_set_encode_rows(FlakeAmdSet *g, const void *rows_dev, int format, int nrows,
                                                  long long row_len, const int *stream_of_row,
                                                  const long long *len_of_row, unsigned char *out, size_t out_size,
                                                  long long *row_whole_bytes, long long *row_tail_bytes);
/* flake_get_streaminfo() for one stream of the set.  The first request after an encode finalises and fetches the
 * digests of ALL streams (one synchronisation); the streams stay open. */
FLAKE_AMD_API int flake_amd_set_get_streaminfo(FlakeAmdSet *g, int stream, FlakeAmdStreaminfo *si);
/*
 * Verification on the device for a set, off by default; returns 0, or -1 without a set.  While on, every frame
 * flake_amd_set_encode writes is checked on the device, before the call returns, to decode to the block it was
 * given and to carry its own stream's frame number (fhip_set_verify / fhip_verify_frames_numbered,
 * include/flakehip.h); with every MD5 mode and both sample widths, and the bytes are the same either way.  A chunk
 * that fails makes flake_amd_set_encode return -1: flake_amd_set_last_error() names the stream, that stream's frame
 * number, the block's index in the call, the status and the subframe, sample and bit; no stream's bookkeeping is
 * committed for the call.  Unless the set was opened with FLAKE_AMD_SET_MD5_HOST or _OFF, the device hashes have
 * already absorbed the chunk and the set refuses further calls, as after an output buffer that was too small.
 *
 * flake_amd_set_last_verify_failure: 1 after a flake_amd_set_encode that failed verification, with the failing
 * frame's stream, its frame number within that stream and its status (FHIP_VERIFY_*) in the outputs (each may be
 * NULL); 0 otherwise, outputs untouched -- so that a caller can decide per file without parsing text.
 */
FLAKE_AMD_API int flake_amd_set_enable_verify(FlakeAmdSet *g, int on);
/* A diagnostic: how many device batches the set has run since it was opened -- one per chunk (at most FLAKE_AMD_BATCH
 * blocks) handed to an encode entry of the HIP layer, whichever entry.  Closing S streams with distinct tails adds
 * ceil(S / FLAKE_AMD_BATCH) through the ragged paths and about S under FLAKE_AMD_SET_RAGGED=0.  -1 without a set. */
FLAKE_AMD_API long long flake_amd_set_device_batches(const FlakeAmdSet *g);
FLAKE_AMD_API int flake_amd_set_last_verify_failure(const FlakeAmdSet *g, int *stream, unsigned *frame_number,
                                                    int *status);
FLAKE_AMD_API const char *flake_amd_set_last_error(const FlakeAmdSet *g);
FLAKE_AMD_API void flake_amd_set_close(FlakeAmdSet *g);

/* ---- decoding ---------------------------------------------------------- */

/*
 * The inverse of flake_amd_write_streaminfo: the 34 bytes of a STREAMINFO block into *si.  The format's sample count
 * has 36 bits and FlakeAmdStreaminfo.samples, which keeps libflake's layout, has 32: si->samples receives the low 32
 * and the return value is the upper four (0 .. 15; 0 for everything flake_amd_write_streaminfo writes).  -1 for a
 * null pointer or a block no stream can carry (sample rate 0 or above 655350, fewer than 4 bits per sample).
 */
FLAKE_AMD_API int flake_amd_read_streaminfo(const unsigned char data34[34], FlakeAmdStreaminfo *si);
/*
 * A SEEKTABLE block's points (the block's content, without the 4-byte metadata header): 18 bytes each -- the first
 * sample of a target frame, the frame's offset in bytes from the first frame's header, the frame's samples.
 * flake_amd_read_seektable stores the first cap points that are not placeholders (sample number all ones) and returns
 * how many such points the block holds; -1 for a null pointer, a length that is no multiple of 18, or points whose
 * sample numbers are not strictly ascending.  flake_amd_seek_lookup returns the index of the last point at or before
 * `sample`, -1 if there is none.  Pure host code.  Nothing in the library trusts a seek point: a caller starts
 * flake_amd_index_frames at the point's byte and falls back to the stream's first frame where that returns -1.
 */
typedef struct FlakeAmdSeekPoint {
    unsigned long long sample;
    unsigned long long offset;
    unsigned frame_samples;
} FlakeAmdSeekPoint;
FLAKE_AMD_API long long flake_amd_read_seektable(const unsigned char *block, size_t bytes, FlakeAmdSeekPoint *points, int cap);
FLAKE_AMD_API long long flake_amd_seek_lookup(const FlakeAmdSeekPoint *points, int n, unsigned long long sample);
/*
 * The inverse of flake_amd_read_seektable: the n points, 18 bytes each and big-endian, followed by `placeholders`
 * placeholder points (sample number all ones, the rest zero), into block[0 .. cap) -- the block's content, without the
 * 4-byte metadata header.  Returns the bytes written, 18 * (n + placeholders); -1 with NOTHING written for a null
 * pointer with a non-zero count, a negative count, sample numbers that are not strictly ascending or equal the
 * placeholder value, a frame_samples above 65535 (the field has 16 bits), a cap that is too small, or n + placeholders
 * above 932067: a metadata block's length has 24 bits and (2^24 - 1) / 18 = 932067.  For every table it accepts,
 * flake_amd_read_seektable returns exactly those points.  Pure host code.
 */
FLAKE_AMD_API long long flake_amd_write_seektable(const FlakeAmdSeekPoint *points, int n, int placeholders,
                                                  unsigned char *block, size_t cap);
/*
 * Seek points while encoding, off by default; with recording off nothing changes, and with it on every frame byte and
 * every STREAMINFO is what it is with it off.  The targets are k * spacing samples, k = 0, 1, 2, ...; a committed block
 * gets a point exactly when at least one target lies in [first, first + its samples), `first` being the stream's sample
 * count before it, and at most one -- so the first block always gets one.  The point is sample = first, offset = the
 * stream's frame bytes before the block, frame_samples = the samples of the block's first frame, read from that frame's
 * header: under variable block size (levels 9-12) a block may be several frames and the point names the first (any
 * frame start is a legal seek point; the inner frames' byte sizes never reach the host).
 *
 * flake_amd_seekpoints / flake_amd_set_seekpoints / flake_amd_recode_set_seekpoints switch recording on with spacing
 * in samples (0: off), after init / open and before the first block: afterwards, and for a null handle, they return
 * -1; else 0.  A set keeps one recorder per stream; a recode set forwards to the stream set inside it.  The getters
 * store the first cap points recorded so far and return how many there are (flake_amd_read_seektable's convention; 0
 * with recording off); -1 for a null handle, a stream index outside the set, a failed stream of a recode set, a
 * negative cap or a null table with cap > 0.  An encode call that returns -1 "with nothing changed" changes no points
 * either; what a single stream or a ragged set call takes back of its bookkeeping after a failure, it takes back of its
 * points.  flake_amd_encode_frame's look-ahead queue records when it flushes.
 *
 * flake_amd_seekpoints_of_frames applies the same rule to a finished stream, each FRAME a block: stream[0 .. bytes)
 * holds nframes frames back to back with the sizes flake_amd_index_frames (or the device's indexer) found, every
 * frame's samples are read from its header against si, and offsets count from stream[0].  It returns the number of
 * points and stores the first cap; -1 for a bad argument (spacing 0 included) or a frame whose header does not parse.
 * Pure host code.
 */
FLAKE_AMD_API int flake_amd_seekpoints(FlakeAmdContext *s, unsigned long long spacing);
FLAKE_AMD_API long long flake_amd_get_seekpoints(const FlakeAmdContext *s, FlakeAmdSeekPoint *p, int cap);
FLAKE_AMD_API int flake_amd_set_seekpoints(FlakeAmdSet *g, unsigned long long spacing);
FLAKE_AMD_API long long flake_amd_set_get_seekpoints(const FlakeAmdSet *g, int stream, FlakeAmdSeekPoint *p, int cap);
FLAKE_AMD_API long long flake_amd_seekpoints_of_frames(const FlakeAmdStreaminfo *si, const unsigned char *stream, size_t bytes,
                                                       const int *frame_sizes, int nframes, unsigned long long spacing,
                                                       FlakeAmdSeekPoint *points, int cap);
/*
 * Frame discovery in a foreign stream, on the CPU (no call into the HIP layer): the sizes of the whole frames that
 * stream[0 .. bytes) begins with, at most cap of them, into frame_sizes; the return value is their count and *consumed
 * (optional) the bytes they cover, so that a caller can feed a file in pieces, each starting where the last one's
 * *consumed ended.  A frame starts at a CANDIDATE -- the sync code, header codes that agree with si (channels, bits per
 * sample, sample rate, a block size within max_block_size), a valid CRC-8, the blocking strategy of the piece's first
 * frame and the expected number: the previous frame's + 1, or + its size in a variable-block-size stream -- and ends at
 * the next candidate for which the CRC-16 of the span holds; a candidate that fails either test is skipped, since audio
 * data may hold a byte sequence that looks like a header.  The last frame ends at `bytes` if its CRC-16 holds there;
 * otherwise (a piece cut inside a frame) it is not counted.  The first frame of a piece may carry any number.
 * Returns -1 when stream[0] does not start a frame (garbage at the start) or for a bad argument.
 */
FLAKE_AMD_API long long flake_amd_index_frames(const FlakeAmdStreaminfo *si, const unsigned char *stream, size_t bytes,
                                               int *frame_sizes, int cap, size_t *consumed);
/*
 * A decoder for one stream on the device (fhip_decode_frames, include/flakehip.h: K7).  flake_amd_decode_open sizes
 * its handle from si (channels, sample rate, bits per sample; blocks up to max_block_size, 65535 when that is 0); the
 * device is FLAKE_AMD_DEVICE and a GPU batch holds up to FLAKE_AMD_BATCH frames (default 1024; fewer for very long
 * blocks), as for encoding.  NULL on failure: flake_amd_decode_last_error(NULL) says why.
 *
 * flake_amd_decode_frames decodes nframes frames, back to back in stream[0 .. bytes) with the sizes
 * flake_amd_index_frames found, into pcm: channel-interleaved int32 with sample_bytes 4, int16_t with 2
 * (bits_per_sample <= 16 only); pcm_cap_samples counts samples per channel.  The blocking strategy and the first
 * number are read from the first frame the decoder ever sees; from then on every frame must carry the number that
 * follows its predecessor's, across calls.  Returns the samples per channel written, or -1:
 * flake_amd_decode_last_error names the frame (counted from the decoder's first), its status (FHIP_VERIFY_*), subframe
 * and bit.  A failed call leaves the decoder's numbering and hash where they were before the failing batch.
 * Everything returned is hashed (md5.c) at the stream's sample width, so that flake_amd_decode_md5 after the last
 * frame is what STREAMINFO's md5sum must be.
 */
typedef struct FlakeAmdDecoder FlakeAmdDecoder;
FLAKE_AMD_API FlakeAmdDecoder *flake_amd_decode_open(const FlakeAmdStreaminfo *si);
FLAKE_AMD_API long long flake_amd_decode_frames(FlakeAmdDecoder *d, const unsigned char *stream, size_t bytes,
                                                const int *frame_sizes, int nframes, void *pcm, int sample_bytes,
                                                size_t pcm_cap_samples);
/*
 * flake_amd_index_frames on the device (fhip_index_frames, include/flakehip.h: K8), on the decoder's handle and against
 * its STREAMINFO: the same sizes, the same count, the same *consumed and the same -1 for every input, good or corrupt.
 * It neither reads nor changes the decoder's numbering or hash.  -2 where the device could not answer (a stream of
 * 2 GiB or more, or a HIP failure: flake_amd_decode_last_error says which); the CPU function still can.
 */
FLAKE_AMD_API long long flake_amd_decode_index(FlakeAmdDecoder *d, const unsigned char *stream, size_t bytes,
                                               int *frame_sizes, int cap, size_t *consumed);
FLAKE_AMD_API int flake_amd_decode_md5(FlakeAmdDecoder *d, unsigned char md5[16]);
FLAKE_AMD_API const char *flake_amd_decode_last_error(const FlakeAmdDecoder *d);
FLAKE_AMD_API void flake_amd_decode_close(FlakeAmdDecoder *d);

/*
 * A decode set: the frames of MANY streams decoded in shared device batches (fhip_decode_frames_segments: K7's segment
 * mode), each stream's MD5 carried on the device (K6's k_md5_ranges, fed on the device by the ranges K7 leaves) -- the
 * counterpart of flake_amd_set_* for decoding.  A folder of ordinary files, one FlakeAmdDecoder after another, is a few
 * dozen frames per launch and one host hash per file; through a set it is FLAKE_AMD_BATCH frames per launch.
 *
 * All streams share like's channels, sample rate and bits per sample; their blocks are at most like->max_block_size
 * (65535 when that is 0).  The blocking strategy and the first number are read PER STREAM from the first frame the set
 * sees of it.  flags: FLAKE_AMD_SET_MD5_HOST (hash on the CPU, on the calling thread: the comparison leg) or
 * FLAKE_AMD_SET_MD5_OFF (no hash); anything else, or both, is an error.  One handle; the device is FLAKE_AMD_DEVICE, a
 * device batch holds up to FLAKE_AMD_BATCH frames (default 1024; fewer for very long blocks).  NULL on failure:
 * flake_amd_decode_set_last_error(NULL) says why.
 *
 * flake_amd_decode_set_frames hands over nruns RUNS: run r is frames_of_run[r] consecutive frames of stream
 * stream_of_run[r]; all frames lie back to back in stream[0 .. bytes) with their frame_sizes (flake_amd_index_frames).
 * A stream may have several runs in a call, in stream order; a run may be empty.  pcm (int32 with sample_bytes 4,
 * int16_t with 2, bits_per_sample <= 16 only; pcm_cap_samples per channel) receives the runs' samples back to back in
 * call order -- as flake_amd_set_encode's `out`, the caller scatters -- and run_samples[r] each run's count.  The call is
 * cut into device batches at frame boundaries, inside a run where that falls; the run's numbering carries over.
 * Returns the samples per channel of the good runs, or -1 with NOTHING changed for a bad argument: a stream index
 * outside the set, frame sizes below 1 or past `bytes`, 2-byte samples above 16 bits, or a run that names a FAILED stream.
 *
 * Failure is per stream, not per call.  A frame that fails (any FHIP_VERIFY_* status; also a frame that does not fit
 * pcm_cap_samples) fails its stream, for good: flake_amd_decode_set_failed returns 1 with the frame, counted from the
 * stream's first, and the status (0: the stream is good; -1: no such stream).  The failing run and that stream's later
 * runs of the call get run_samples[r] = -1; their samples are unspecified, and what lies behind them in pcm is no
 * longer where the counts alone put it: flake_amd_decode_set_run_offsets gives every run's first sample in pcm for the
 * last call (-1 for a run without one; returns the number of runs).  Every other stream is committed as if nothing had
 * happened.  (A failing run's samples are NOT kept as a hole of their size -- a size nobody knows once a header is
 * broken: the next device batch's samples begin behind the last good segment's.  Hence the offsets entry.)
 *
 * Two rules are held on the CPU where the device has no predecessor to compare with.  A fixed-block stream keeps ONE
 * block size from segment to segment: a frame shorter than it ends the stream, and a frame behind such a frame fails
 * with NUMBER even where a device batch or a run was cut between the two -- there the frame BEHIND the short one is
 * named, inside one segment the short one itself.  A variable-block-size stream's later run in a device batch is held
 * to the sample number that its earlier run's samples lead to.  A stream whose first header the CPU cannot read is
 * still handed to the device, which names what is wrong with it (CRC8 for a CRC-8, as for any later frame).
 *
 * flake_amd_decode_set_md5: the digest of everything stream `stream` has returned -- what its STREAMINFO's md5sum must
 * be after the last frame.  The first request after a call finalises ALL streams' digests (one launch, one copy, one
 * synchronisation); later requests are copies.  -1 for a failed stream or a set opened with FLAKE_AMD_SET_MD5_OFF.
 * flake_amd_decode_set_device_batches: device batches run so far (-1 without a set).
 *
 * Measured (profiles/decode_set_bench.txt, 4096 stereo 16-bit frames of 4096): 256 streams of 16 frames take 77.7 ms
 * through one set, 3704 ms through one FlakeAmdDecoder each and 134.5 ms as one stream through one decoder.  A lane
 * hashes 87 MB/s, a CPU core about 1 GB/s: the device hash loses to FLAKE_AMD_SET_MD5_HOST up to 32 streams (16 streams:
 * 259 against 134.5 ms) and wins from 64 on; below a few dozen streams open the set with FLAKE_AMD_SET_MD5_HOST.
 */
typedef struct FlakeAmdDecodeSet FlakeAmdDecodeSet;
FLAKE_AMD_API FlakeAmdDecodeSet *flake_amd_decode_set_open(const FlakeAmdStreaminfo *like, int nstreams, unsigned flags);
FLAKE_AMD_API long long flake_amd_decode_set_frames(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run,
                                                    const int *frames_of_run, const unsigned char *stream, size_t bytes,
                                                    const int *frame_sizes, void *pcm, int sample_bytes,
                                                    size_t pcm_cap_samples, long long *run_samples);
FLAKE_AMD_API int flake_amd_decode_set_run_offsets(const FlakeAmdDecodeSet *g, long long *offsets, int cap);
FLAKE_AMD_API int flake_amd_decode_set_md5(FlakeAmdDecodeSet *g, int stream, unsigned char md5[16]);
FLAKE_AMD_API int flake_amd_decode_set_failed(const FlakeAmdDecodeSet *g, int stream, long long *frame, int *status);
FLAKE_AMD_API long long flake_amd_decode_set_device_batches(const FlakeAmdDecodeSet *g);
/*
 * Frame discovery for many files in ONE device call (K8) on the set's handle: range r is stream[range_first[r] ..
 * range_first[r + 1]) (nranges + 1 offsets, from 0, not decreasing, the last one the byte count), one file's frames
 * from its first header on.  Exactly
 *   for r in ranges: range_frames[r] = flake_amd_index_frames(si, range r, frame_sizes + frames so far,
 *                                                             cap - frames so far, &range_consumed[r])
 * where si is the set's format with the call's max_block_size (the files' STREAMINFO value; 0: not checked) -- a call holds one format, so files whose max_block_size differ go through calls of their own --
 * with the ranges' sizes back to back in frame_sizes: a range that is refused (-1) takes no room, ranges behind the
 * one that cap cut get 0.  Returns 0, -1 for a bad argument, -2 where the device could not answer (2 GiB or more in
 * one call, or a HIP failure: flake_amd_decode_set_last_error says which).  The set's streams are not touched.
 */
FLAKE_AMD_API int flake_amd_decode_set_index(FlakeAmdDecodeSet *g, unsigned max_block_size, const unsigned char *stream,
                                             const size_t *range_first, int nranges, int *frame_sizes, int cap,
                                             long long *range_frames, size_t *range_consumed);
/*
 * WINDOWS of samples out of many streams in shared device batches -- seeking.  Window w is count[w] samples per channel
 * from absolute sample first_sample[w] of its stream, asked of a RUN: frames_of_win[w] consecutive frames of that stream,
 * starting at any frame (a whole file's, or what flake_amd_index_frames found from a seek point on), all runs back to
 * back in stream / frame_sizes as for flake_amd_decode_set_frames.  fixed_block_size[w] is the stream's STREAMINFO block
 * size where minimum and maximum agree, else 0 (the run's first frame's size then stands for it; a variable-block-size
 * stream carries sample numbers and needs neither).  The frames that overlap each window are found on the host from
 * their headers (bisection: the numbers increase), only their bytes are uploaded, and the device delivers of them
 * exactly the window (K7's window mode): nothing is trimmed afterwards.
 *
 * Stateless, like flake_amd_decode_set_index: the call runs on the set's handle with the set's format and neither
 * reads nor changes any stream's numbering, hash or failed state.  The windows' samples lie back to back in pcm, in
 * call order (sample_bytes 4 or 2 as for flake_amd_decode_set_frames).  win_samples[w] is what window w delivers: count[w],
 * less where the run ends inside the window, 0 where the window begins before the run's first frame or at or behind
 * its end, or count[w] is 0.  win_status[w] is 0 for a good window, else the FHIP_VERIFY_* status of its first failing
 * frame (HEADER also where the search met something that is no header of the stream); such a window has
 * win_samples[w] = -1 and keeps the room it ASKED for, count[w] samples of unspecified content, and every other window is
 * delivered as if nothing had happened.  *frames_decoded (optional) is the number of frames handed to the device.
 * Returns the good windows' samples; -1 with nothing written for a bad argument: sizes that do not add up inside bytes, a
 * negative count, 2-byte samples above 16 bits, pcm_cap_samples below the sum of the counts.
 */
FLAKE_AMD_API long long flake_amd_decode_set_windows(FlakeAmdDecodeSet *g, int nwin, const int *frames_of_win,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count,
        void *pcm, int sample_bytes, size_t pcm_cap_samples,
        long long *win_samples, int *win_status, long long *frames_decoded);
/*
 * The same windows as a padded planar batch that STAYS ON THE DEVICE, for a consumer there (a training loop that crops a
 * corpus): window w is row w of dev_rows, DEVICE memory on the set's device of nwin x channels x row_len elements laid
 * out [window][channel][time].  row_format says what an element is: FLAKE_AMD_ROWS_I32 the sample, FLAKE_AMD_ROWS_I16
 * the sample as int16_t (sets of at most 16 bits), FLAKE_AMD_ROWS_F32 (float)sample * 2^-(bits_per_sample - 1), a value in
 * [-1, 1) that is exact up to 24 bits and rounded once, to nearest even, above.  Arguments, selection, batches,
 * win_samples, win_status, *frames_decoded and the return value are flake_amd_decode_set_windows', value for value.
 * No sample crosses to the host: each batch's windows are re-laid on the device behind the decoder (K10), a window
 * that a batch cuts continuing at the column it had reached.
 *
 * On return the rows are complete, nothing is pending, and every element of all nwin rows that no good window's
 * delivered samples cover is zero: the padding behind a window, the row of a window that delivers nothing, and the whole
 * row of a window that failed -- also where an earlier batch had written part of it.  (The destination is zeroed on the
 * device before the first batch and a failed window's row again at the end.)  The library writes on its handle's
 * stream: work of the caller's that still uses dev_rows on another stream must have finished before the call.
 * Returns -1 with nothing written to dev_rows for what flake_amd_decode_set_windows refuses, a count[w] above row_len,
 * row_len < 1, a null dev_rows with nwin > 0, an unknown row_format or FLAKE_AMD_ROWS_I16 above 16 bits.  Stateless like
 * its sibling.
 */
#define FLAKE_AMD_ROWS_I32 0
#define FLAKE_AMD_ROWS_I16 1
#define FLAKE_AMD_ROWS_F32 2
FLAKE_AMD_API long long flake_amd_decode_set_windows_rows(FlakeAmdDecodeSet *g, int nwin, const int *frames_of_win,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count,
        void *dev_rows, int row_format, long long row_len,
        long long *win_samples, int *win_status, long long *frames_decoded);
/*
 * HELD STREAMS: a corpus that stays on the device.  The set owns one store of capacity_bytes of device memory, streams
 * are appended to it and indexed where they lie, and windows are then asked for by (held stream, first_sample, count):
 * no stream byte crosses the link again, a call uploads only its tables and 12 bytes per selected frame.  The set's
 * handle, format and FLAKE_AMD_BATCH apply.
 *
 * flake_amd_decode_set_hold allocates the store, once per set: -1 on a second call, for capacity_bytes 0 or when the
 * allocation fails.
 *
 * flake_amd_decode_set_hold_add appends ranges as flake_amd_decode_set_index takes them -- one file each, from its first
 * frame header on -- and gives every range the set's next id in held_ids[r], a range K8 refuses (-1) included: such a
 * held stream has 0 frames and its windows deliver 0.  fixed_block_size[r] is STREAMINFO's block size where minimum and
 * maximum agree, else 0.  The bytes are uploaded behind what the store holds, K8 runs on the resident copy, every
 * frame's header is read on the device (k_frame_heads), and the frames' sizes and heads come back into the set's table,
 * with one synchronisation (a second beyond 65536 frames in one call).  Returns the frames found; -1 with nothing
 * changed for a bad argument, a set without a store, 2 GiB or more in one call (K8's limit), no room in the store or a
 * HIP failure.  Files whose max_block_size differ go through calls of their own.
 *
 * flake_amd_decode_set_held_windows / _held_windows_rows are flake_amd_decode_set_windows / _windows_rows, value for
 * value, with window w asked of the whole run of held stream held_of_win[w]: the frames and sizes hold_add found, the
 * stream's fixed_block_size, the samples or rows, win_samples, win_status, *frames_decoded, the return value, the room a
 * failed window keeps and the zeroing rule of the rows.  Selection is the same bisection, over the table's heads instead
 * of the bytes: it probes the same frames in the same order.  Stateless like their siblings; also -1 for an id outside
 * the set's held streams.
 *
 * flake_amd_decode_set_held_info: a held stream's frames, the samples its good headers add up to and its bytes (any
 * pointer may be null); -1 for an id the set does not have.  flake_amd_decode_set_held_stats: out[0] bytes resident,
 * out[1] frames in the table, out[2] bytes uploaded by hold_add, out[3] bytes uploaded by held window calls.
 * flake_amd_decode_set_close frees the store.  Streams cannot be removed or replaced.
 */
FLAKE_AMD_API int flake_amd_decode_set_hold(FlakeAmdDecodeSet *g, size_t capacity_bytes);
FLAKE_AMD_API long long flake_amd_decode_set_hold_add(FlakeAmdDecodeSet *g, unsigned max_block_size,
        const unsigned char *stream, const size_t *range_first, int nranges, const unsigned *fixed_block_size,
        int *held_ids);
FLAKE_AMD_API long long flake_amd_decode_set_held_windows(FlakeAmdDecodeSet *g, int nwin, const int *held_of_win,
        const unsigned long long *first_sample, const long long *count,
        void *pcm, int sample_bytes, size_t pcm_cap_samples,
        long long *win_samples, int *win_status, long long *frames_decoded);
FLAKE_AMD_API long long flake_amd_decode_set_held_windows_rows(FlakeAmdDecodeSet *g, int nwin, const int *held_of_win,
        const unsigned long long *first_sample, const long long *count,
        void *dev_rows, int row_format, long long row_len,
        long long *win_samples, int *win_status, long long *frames_decoded);
FLAKE_AMD_API int flake_amd_decode_set_held_info(const FlakeAmdDecodeSet *g, int id, long long *frames, long long *samples,
                                                 long long *bytes);
FLAKE_AMD_API int flake_amd_decode_set_held_stats(const FlakeAmdDecodeSet *g, long long out[4]);
/*
 * SPAN ROWS: every window of row_len samples, hop samples apart, of a span of a stream -- with every frame decoded once.
 * What a caller gets that walks whole recordings in consecutive (hop == row_len), overlapping (hop < row_len) or spaced
 * (hop > row_len) chunks; asked as one window per chunk, a frame that two chunks touch is decoded twice.
 *
 * A call has one row_len >= 1 and one hop in 1 .. 2^31 - 1 and names spans (stream, first_sample[s], count[s] >= 0) as
 * the windows calls name windows: _span_rows of runs the caller brings (flake_amd_decode_set_windows_rows' arguments),
 * _held_span_rows of held streams by id.  Span s has
 *   R_s = 0 for count[s] == 0, else min(ceil(count[s] / hop), 1 + ceil(max(count[s] - row_len, 0) / hop))
 * rows (flake_amd_span_rows_count; -1 for a negative count, row_len < 1 or a hop out of range): the rows j with
 * j * hop < count[s] whose predecessor has not reached the span's end.  The spans' rows lie span after span in dev_rows,
 * [row][channel][row_len] of row_format as the windows' rows: span_first_row[s] is span s's first row and
 * span_first_row[nspans] the call's rows, which is also what is returned.
 *
 * A span is decoded as ONE window: selection, batches, the held gather and the placement are the window calls', and
 * *frames_decoded counts every selected frame once.  With D_s <= count[s] the samples that window delivers (cut at the
 * stream's end; 0 behind it) and x_s those samples, row span_first_row[s] + j holds x_s[j * hop + i] at column i where
 * j * hop + i < D_s and zero elsewhere, row_samples[...] = clamp(D_s - j * hop, 0, row_len) and span_status[s] = 0.  A
 * span fails as the window would -- any of its frames on the device, a header the planner needs -- and fails whole and
 * alone: all its rows are zero, their row_samples -1, span_status[s] the window's status.  (K13 lays each batch's
 * samples into every row they belong to behind the decoder; all the call's rows are zeroed before the first batch and a
 * failed span's again at the end.)  Rows behind the call's are never touched.  The stream rule is the windows' rows'.
 *
 * Returns -1 with nothing written for what the window rows calls refuse of their stream arguments, a negative count,
 * hop < 1 or above 2^31 - 1, row_len < 1, an unknown row_format, FLAKE_AMD_ROWS_I16 above 16 bits, null tables, and for
 * more rows than rows_cap (the rows dev_rows and row_samples have room for) or than 2^31 - 1.  Stateless.
 */
FLAKE_AMD_API long long flake_amd_span_rows_count(long long count, long long row_len, long long hop);
FLAKE_AMD_API long long flake_amd_decode_set_span_rows(FlakeAmdDecodeSet *g, int nspans, const int *frames_of_span,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count, long long hop,
        void *dev_rows, int row_format, long long row_len, long long rows_cap,
        int *span_first_row, long long *row_samples, int *span_status, long long *frames_decoded);
FLAKE_AMD_API long long flake_amd_decode_set_held_span_rows(FlakeAmdDecodeSet *g, int nspans, const int *held_of_span,
        const unsigned long long *first_sample, const long long *count, long long hop,
        void *dev_rows, int row_format, long long row_len, long long rows_cap,
        int *span_first_row, long long *row_samples, int *span_status, long long *frames_decoded);
FLAKE_AMD_API const char *flake_amd_decode_set_last_error(const FlakeAmdDecodeSet *g);
FLAKE_AMD_API void flake_amd_decode_set_close(FlakeAmdDecodeSet *g);

/* ---- recoding: FLAC in, FLAC out, the PCM never leaving the device ------ */

/*
 * A recode set joins a decode set to a stream set ON THE DEVICE: the frames of many streams go in as
 * flake_amd_decode_set_frames takes them, and what comes out is, for every stream, byte for byte what a FlakeAmdSet at
 * enc_like's parameters writes for that stream's samples -- whole blocks while frames arrive, the tail at the end,
 * STREAMINFO included.  The decoder's blocks (1152, 4608, variable, whatever the source used) are re-cut into the
 * encoder's block size by a gather kernel (K9, fhip_frames_packed_gather); a stream's samples that do not fill a block
 * wait in a device carry (below one block per stream) for the next call.  The samples cross the link in neither
 * direction and are hashed once: STREAMINFO's md5sum is the DECODE side's digest (K6 over the ranges K7 left), the
 * encode set inside runs without a hash.  Comparing that digest with the source file's is the caller's.
 *
 * flake_amd_recode_set_open: all streams share src_like's channels, sample rate and bits per sample, which must equal
 * enc_like's; their source blocks are at most src_like->max_block_size (65535 when 0).  flags: FLAKE_AMD_SET_VBS is
 * required exactly when enc_like has variable block size (levels 9-12); FLAKE_AMD_SET_MD5_OFF leaves md5sum zero;
 * FLAKE_AMD_SET_MD5_HOST is refused (there is no PCM on the host), as is an encoder block size above 16384 (the tails
 * need the ragged packed path).  Two handles, a decode one and an encode one, each
 * with FLAKE_AMD_BATCH frames / blocks per device batch.  NULL on failure: flake_amd_recode_set_last_error(NULL).
 *
 * flake_amd_recode_set_frames: the input is flake_amd_decode_set_frames' (runs of frames, back to back in `stream`).
 * `out` receives the whole blocks the call completes, back to back; block b of them belongs to stream block_stream[b]
 * and is block_bytes[b] bytes (all its frames' under variable block size), so the caller scatters; *nblocks is their
 * count.  A stream's blocks come in stream order; the order is otherwise unspecified.  Returns the bytes written, or
 * -1.  out_size and block_cap must reach flake_amd_recode_set_out_bound(g, frames of the call): the carries plus that
 * many source blocks of the largest size, each block at the largest VERBATIM frame (a full header, a byte per subframe,
 * the samples, the CRC-16; eight of them under variable block size).  Below it, or with a stream index outside the set, a run
 * that names a failed stream, bad frame sizes, or after flake_amd_recode_set_finish, the call returns -1 with NOTHING
 * changed.
 *
 * Failure is per stream, as in a decode set: a frame that fails fails its stream for good
 * (flake_amd_recode_set_failed: 1 with the frame, counted from the stream's first, and its FHIP_VERIFY_* status).
 * Blocks of it already returned stand; nothing further of it is encoded, neither from the failing run on nor at the
 * end, and it has no STREAMINFO.  Every other stream is unaffected.  A device error, or a verification failure on the
 * encode side, makes the call return -1 and the set refuse further calls.
 *
 * flake_amd_recode_set_finish: every good stream's carry is encoded as its tail through the ragged path
 * (flake_amd_set_encode_ragged's: one device batch per FLAKE_AMD_BATCH tails); outputs as above, bound
 * flake_amd_recode_set_out_bound(g, -1).  The set takes no more frames afterwards.
 * flake_amd_recode_set_get_streaminfo: the new STREAMINFO of a good stream (-1 for a failed one).
 * flake_amd_recode_set_enable_verify: the inner set's flake_amd_set_enable_verify -- K5 checks the new frames against
 * the gathered PCM where it lies.  flake_amd_recode_set_device_batches: the decode and the encode batches so far.
 * One format per set; other metadata blocks, int16 device PCM and overlapping a batch's encode with the next batch's
 * decode are out of scope.
 */
typedef struct FlakeAmdRecodeSet FlakeAmdRecodeSet;
FLAKE_AMD_API FlakeAmdRecodeSet *flake_amd_recode_set_open(const FlakeAmdStreaminfo *src_like, const FlakeAmdContext *enc_like,
                                                           int nstreams, unsigned flags);
FLAKE_AMD_API long long flake_amd_recode_set_frames(FlakeAmdRecodeSet *g, int nruns, const int *stream_of_run,
                                                    const int *frames_of_run, const unsigned char *stream, size_t bytes,
                                                    const int *frame_sizes, unsigned char *out, size_t out_size,
                                                    int *block_stream, int *block_bytes, int block_cap, int *nblocks);
/* nframes >= 0: the bound of a flake_amd_recode_set_frames call of that many frames, as the set stands; -1: of
 * flake_amd_recode_set_finish.  Either output may be NULL.  0, or -1 without a set. */
FLAKE_AMD_API int flake_amd_recode_set_out_bound(const FlakeAmdRecodeSet *g, long long nframes, size_t *bytes, long long *blocks);
FLAKE_AMD_API long long flake_amd_recode_set_finish(FlakeAmdRecodeSet *g, unsigned char *out, size_t out_size,
                                                    int *block_stream, int *block_bytes, int block_cap, int *nblocks);
FLAKE_AMD_API int flake_amd_recode_set_get_streaminfo(FlakeAmdRecodeSet *g, int stream, FlakeAmdStreaminfo *si);
FLAKE_AMD_API int flake_amd_recode_set_failed(const FlakeAmdRecodeSet *g, int stream, long long *frame, int *status);
FLAKE_AMD_API int flake_amd_recode_set_device_batches(const FlakeAmdRecodeSet *g, long long *decode, long long *encode);
FLAKE_AMD_API int flake_amd_recode_set_enable_verify(FlakeAmdRecodeSet *g, int on);
/* Seek points of the NEW streams (see flake_amd_seekpoints above): the inner stream set's recorders. */
FLAKE_AMD_API int flake_amd_recode_set_seekpoints(FlakeAmdRecodeSet *g, unsigned long long spacing);
FLAKE_AMD_API long long flake_amd_recode_set_get_seekpoints(const FlakeAmdRecodeSet *g, int stream, FlakeAmdSeekPoint *p, int cap);
FLAKE_AMD_API const char *flake_amd_recode_set_last_error(const FlakeAmdRecodeSet *g);
FLAKE_AMD_API void flake_amd_recode_set_close(FlakeAmdRecodeSet *g);

/* Deterministic synthetic PCM, channel-interleaved int32 as
 * flake_encode_frame() expects: nframes blocks of n samples per channel,
 * starting at absolute frame index first_frame. */
FLAKE_AMD_API void flake_amd_synth_pcm(int32_t *pcm, int64_t first_frame, int nframes,
                                       int n, int channels, int bps);

#ifdef __cplusplus
}
#endif
#endif /* FLAKE_AMD_H */
