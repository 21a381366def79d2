/* host_internal.h -- shared by the host C sources; not installed. */
#ifndef FLAKE_AMD_HOST_INTERNAL_H
#define FLAKE_AMD_HOST_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "../csrc/flac_header.h"

typedef struct fa_md5 {
    uint32_t h[4];
    uint64_t len;
    uint8_t buf[64];
    int fill;
} fa_md5;

void fa_md5_init(fa_md5 *m);
void fa_md5_update(fa_md5 *m, const uint8_t *data, size_t n);
void fa_md5_final(const fa_md5 *m, uint8_t out[16]);
void fa_md5_pcm(fa_md5 *m, const int32_t *pcm, size_t nvalues, int bps);
void fa_md5_pcm16(fa_md5 *m, const int16_t *pcm, size_t nvalues, int bps);

/* The frame-header predicate of csrc/flac_header.h held against a STREAMINFO (flake_decode.c): 0 and *h for a header
 * of that stream at d[0 .. avail), else -1. */
struct FlakeAmdStreaminfo;
int fa_parse_header(const struct FlakeAmdStreaminfo *si, const unsigned char *d, size_t avail, flac_header *h);

/* K8 for the decoder and the decode set (flake_decode.c): fhip_index_frames over nranges ranges of stream, the answers
 * in the host layer's types.  0, -1 for a bad argument, -2 where the device could not answer (err says why). */
struct fhip_ctx;
int fa_index_ranges(struct fhip_ctx *hip, unsigned max_block_size, const unsigned char *stream, const size_t *range_first,
                    int nranges, int *frame_sizes, int cap, long long *range_frames, size_t *range_consumed, char *err,
                    size_t err_len);

/* Which of a chunk's cnt blocks the verifier's frame index (it counts the chunk's frames) lies in: block b holds
 * block_frames[b] frames, one each when the table is null.  -1: none -- an index below 0 or past the chunk's frames;
 * an entry below 1 ends the search (nothing behind a block that was not encoded can be placed). */
static inline int fa_block_of_frame(long long frame, const int32_t *block_frames, int cnt)
{
    long long at = 0;
    for (int b = 0; b < cnt && frame >= 0; b++) {
        const int nf = block_frames ? block_frames[b] : 1;
        if (nf < 1) break;
        at += nf;
        if (frame < at) return b;
    }
    return -1;
}

/* ---- what a recode set (flake_recode_set.c) opens inside a stream set and a decode set ---- */

/* An encode call's samples as gather pieces from device memory instead of a host buffer (flake_set.c).  pieces tile the
 * call's samples (all blocks back to back); each chunk of the call gathers its part of them (fa_rc_slice into work,
 * which has room for npieces; cur is that walk's place, 0 before the call).
 * The second kind, rows (non-null: flake_amd_set_encode_rows): the samples are row pieces of a planar batch on the
 * device, converted by K12; row_pieces tile the call's samples as pieces do, each chunk converts its part of them
 * (fa_rows_slice into row_work, room for npieces), and the gather fields are unused. */
struct fhip_gather_piece;
struct fhip_rows_in;
struct fhip_row_piece;
typedef struct fa_set_source {
    const struct fhip_gather_piece *pieces;
    int npieces;
    const int32_t *src0, *src1;   /* device memory, capacities in samples per channel */
    int64_t src0_cap, src1_cap;
    struct fhip_gather_piece *work;
    int cur;
    const struct fhip_rows_in *rows;
    const struct fhip_row_piece *row_pieces;
    struct fhip_row_piece *row_work;
} fa_set_source;
struct FlakeAmdSet;
/* flake_amd_set_encode / flake_amd_set_encode_ragged (every block short, one per stream) with int32 samples from src;
 * not for a set that hashes on the host.  The ragged form needs the ragged packed path: -1 where the set has none. */
long long fa_set_encode_from(struct FlakeAmdSet *g, fa_set_source *src, int nblocks, int block_size,
                             const int *stream_of_block, unsigned char *out, size_t out_size, int *frame_sizes);
long long fa_set_encode_short_from(struct FlakeAmdSet *g, fa_set_source *src, int nblocks, const int *block_sizes,
                                   const int *stream_of_block, unsigned char *out, size_t out_size, int *frame_sizes);
struct fhip_ctx *fa_set_handle(struct FlakeAmdSet *g);
int fa_set_max_batch(const struct FlakeAmdSet *g);

/* flake_amd_decode_set_frames with the samples LEFT ON THE DEVICE (flake_decode_set.c): every device batch decodes to
 * dev_pcm[0 ..) (int32, dev_cap_samples per channel: fa_decode_set_batch_samples() always suffices) and, once the set
 * has judged its segments, is handed to fn: segment k is seg_samples[k] samples of stream seg_stream[k] at seg_start[k],
 * good where seg_ok[k] -- a segment that is not fails its stream, as the set has already noted.  fn returns below 0 to
 * stop the call (it returns -1 then).  The next batch overwrites dev_pcm. */
struct FlakeAmdDecodeSet;
typedef int (*fa_ds_batch_fn)(void *user, int nsegs, const int32_t *seg_stream, const int64_t *seg_start,
                              const int64_t *seg_samples, const unsigned char *seg_ok);
long long fa_decode_set_frames_keep(struct FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run,
                                    const int *frames_of_run, const unsigned char *stream, size_t bytes,
                                    const int *frame_sizes, int32_t *dev_pcm, size_t dev_cap_samples,
                                    long long *run_samples, fa_ds_batch_fn fn, void *user);
size_t fa_decode_set_batch_samples(const struct FlakeAmdDecodeSet *g);     /* frames per batch x the largest block */
int fa_decode_set_max_batch(const struct FlakeAmdDecodeSet *g);
int fa_decode_set_max_block(const struct FlakeAmdDecodeSet *g);

#endif
