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

#endif
