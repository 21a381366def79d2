/*
 * flake_recode_set.c -- a recode set: FLAC frames of many streams in, FLAC frames at other parameters out, the PCM never
 * leaving the device.  It owns a decode set (flake_decode_set.c) with the keep-on-device destination and a stream set
 * (flake_set.c) whose encode entries take their samples as gather pieces; between the two sits the planner
 * (recode_plan.h), which re-cuts each decode batch's segments, with every stream's carry from the batches before, into
 * the encoder's blocks as K9's piece tables.
 *
 * Per decode batch: K7 (and K6: the streams' MD5s, the only hash taken) on the decode handle, which synchronises; the
 * plan on the host; then on the encode handle the whole blocks (fhip_frames_packed_gather in front of the packed path,
 * one device batch per FLAKE_AMD_BATCH blocks) and the new carries (fhip_gather_spans_dev).  The carries are
 * double-buffered: a step reads carry buffer `cur` and the decoded buffer and writes carry buffer `cur ^ 1`, so no gather
 * reads what it or the other writes.  The encode side starts only after the decode call has returned.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"
#include "flakehip.h"
#include "host_internal.h"
#include "recode_plan.h"

struct FlakeAmdRecodeSet {
    FlakeAmdDecodeSet *dec;
    FlakeAmdSet *enc;
    int nstreams, block, vbs, finished, broken;
    unsigned flags;
    int per_block;                /* bytes one block's frames take at most */
    int src_max_block;
    int32_t *d_dec;               /* device: one decode batch's samples */
    size_t dec_cap;
    int32_t *d_carry[2];          /* device: the carries, dense and in stream order; `cur` is the valid one */
    size_t carry_cap;
    int cur;
    fa_rc_stream *st;
    fa_rc_plan plan;
    int plan_blocks;              /* room in plan.block_stream */
    fhip_gather_piece *work;      /* a chunk's slice of the block pieces */
    int32_t *tail_sizes, *tail_streams;
    int *fsz;                     /* [plan_blocks] the bytes of a step's blocks */
    long long *run_samples;
    int run_cap;
    /* the call in progress: where its blocks go */
    unsigned char *out;
    size_t out_size, out_at;
    int *block_stream, *block_bytes;
    int block_cap, nblocks;
    char err[384];
};

static char g_open_err[384];

#define RC_FAIL(...) do { snprintf(g->err, sizeof g->err, __VA_ARGS__); return -1; } while (0)

FLAKE_AMD_API const char *flake_amd_recode_set_last_error(const FlakeAmdRecodeSet *g) { return g ? g->err : g_open_err; }

FLAKE_AMD_API void flake_amd_recode_set_close(FlakeAmdRecodeSet *g)
{
    if (!g) return;
    if (g->enc) flake_amd_set_close(g->enc);                  /* (waits for its handle's streams) */
    if (g->dec) flake_amd_decode_set_close(g->dec);
    if (g->d_dec) fhip_device_free(g->d_dec);
    if (g->d_carry[0]) fhip_device_free(g->d_carry[0]);
    if (g->d_carry[1]) fhip_device_free(g->d_carry[1]);
    free(g->st); free(g->plan.block_pieces); free(g->plan.carry_pieces); free(g->plan.block_stream); free(g->plan.first);
    free(g->plan.order); free(g->plan.avail); free(g->work); free(g->tail_sizes); free(g->tail_streams); free(g->fsz);
    free(g->run_samples);
    free(g);
}

FLAKE_AMD_API FlakeAmdRecodeSet *flake_amd_recode_set_open(const FlakeAmdStreaminfo *src_like, const FlakeAmdContext *enc_like,
                                                           int nstreams, unsigned flags)
{
    g_open_err[0] = 0;
#define OPEN_FAIL(...) do { snprintf(g_open_err, sizeof g_open_err, __VA_ARGS__); flake_amd_recode_set_close(g); return NULL; } while (0)
    FlakeAmdRecodeSet *g = NULL;
    if (!src_like || !enc_like) OPEN_FAIL("flake_amd_recode_set_open: null argument");
    if (flags & FLAKE_AMD_SET_MD5_HOST)
        OPEN_FAIL("flake_amd_recode_set_open: FLAKE_AMD_SET_MD5_HOST is not supported: there is no PCM on the host to hash");
    if (flags & ~(FLAKE_AMD_SET_MD5_OFF | FLAKE_AMD_SET_VBS)) OPEN_FAIL("flake_amd_recode_set_open: unknown flags");
    if ((int)src_like->channels != enc_like->channels || (int)src_like->sample_rate != enc_like->sample_rate ||
        (int)src_like->bits_per_sample != enc_like->bits_per_sample)
        OPEN_FAIL("flake_amd_recode_set_open: the source format (%u channels, %u Hz, %u bits) is not the encoder's (%d, %d, %d)",
                  src_like->channels, src_like->sample_rate, src_like->bits_per_sample, enc_like->channels,
                  enc_like->sample_rate, enc_like->bits_per_sample);
    if (nstreams < 1 || nstreams > (1 << 20)) OPEN_FAIL("flake_amd_recode_set_open: nstreams out of range");
    if (enc_like->params.block_size > 16384)
        OPEN_FAIL("flake_amd_recode_set_open: block sizes above 16384 are not supported (the tails need the ragged packed path)");
    g = (FlakeAmdRecodeSet *)calloc(1, sizeof *g);
    if (!g) OPEN_FAIL("flake_amd_recode_set_open: out of host memory");
    g->nstreams = nstreams;
    g->flags = flags;
    g->vbs = (flags & FLAKE_AMD_SET_VBS) != 0;
    /* the samples are hashed once, on the decode side; the encode set hashes nothing */
    g->enc = flake_amd_set_open(enc_like, nstreams, (flags & FLAKE_AMD_SET_VBS) | FLAKE_AMD_SET_MD5_OFF);
    if (!g->enc) OPEN_FAIL("flake_amd_recode_set_open: %s", flake_amd_set_last_error(NULL));
    g->dec = flake_amd_decode_set_open(src_like, nstreams, flags & FLAKE_AMD_SET_MD5_OFF);
    if (!g->dec) OPEN_FAIL("flake_amd_recode_set_open: %s", flake_amd_decode_set_last_error(NULL));
    g->block = enc_like->params.block_size;
    g->src_max_block = fa_decode_set_max_block(g->dec);
    {
        const int bps = enc_like->bits_per_sample, n = g->block, ch = enc_like->channels;      /* encode.c:521-527 */
        const int verbatim = ch == 2 ? 16 + ((n * (bps + bps + 1) + 7) >> 3) : 16 + ((n * ch * bps + 7) >> 3);
        /* That is the size above which a block is written again as VERBATIM, not the largest frame: the VERBATIM frame
         * itself is its header (16 bytes at most: 4, a number of up to 7, 2 of block size, 2 of sample rate, the CRC-8),
         * a byte per subframe, the samples and the CRC-16.  With eight channels that is above `verbatim` as soon as the
         * header takes 7 bytes (8 x 24 bits, blocks of 16: 401 against 400).  Variable block size: up to eight frames,
         * each with its own header and rounding. */
        const int frames = g->vbs ? 8 : 1;
        g->per_block = (verbatim - 16) + frames * (16 + ch + 2) + (frames - 1);
    }
    const size_t ns = (size_t)nstreams, nch = (size_t)enc_like->channels;
    const size_t segs = (size_t)fa_decode_set_max_batch(g->dec);
    g->dec_cap = fa_decode_set_batch_samples(g->dec);
    g->carry_cap = ns * (size_t)g->block;
    /* a step's blocks: what the carries and one decode batch hold */
    const size_t pb = (g->carry_cap + g->dec_cap) / (size_t)g->block + 1;
    if (pb > 0x7fffffff) OPEN_FAIL("flake_amd_recode_set_open: the block size is too small for this source");
    g->plan_blocks = (int)pb;
    g->d_dec = (int32_t *)fhip_device_alloc(g->dec_cap * nch * sizeof(int32_t));
    g->d_carry[0] = (int32_t *)fhip_device_alloc(g->carry_cap * nch * sizeof(int32_t));
    g->d_carry[1] = (int32_t *)fhip_device_alloc(g->carry_cap * nch * sizeof(int32_t));
    if (!g->d_dec || !g->d_carry[0] || !g->d_carry[1]) OPEN_FAIL("flake_amd_recode_set_open: out of device memory");
    g->st = (fa_rc_stream *)calloc(ns, sizeof *g->st);
    g->plan.block_pieces = (fhip_gather_piece *)calloc(ns + segs, sizeof(fhip_gather_piece));
    g->plan.carry_pieces = (fhip_gather_piece *)calloc(ns + segs, sizeof(fhip_gather_piece));
    g->plan.block_stream = (int32_t *)calloc(pb, sizeof(int32_t));
    g->plan.first = (int32_t *)calloc(ns + 1, sizeof(int32_t));
    g->plan.order = (int32_t *)calloc(segs, sizeof(int32_t));
    g->plan.avail = (long long *)calloc(ns, sizeof(long long));
    g->work = (fhip_gather_piece *)calloc(ns + segs, sizeof(fhip_gather_piece));
    g->tail_sizes = (int32_t *)calloc(ns, sizeof(int32_t));
    g->tail_streams = (int32_t *)calloc(ns, sizeof(int32_t));
    g->fsz = (int *)calloc(pb > ns ? pb : ns, sizeof(int));
    if (!g->st || !g->plan.block_pieces || !g->plan.carry_pieces || !g->plan.block_stream || !g->plan.first ||
        !g->plan.order || !g->plan.avail || !g->work || !g->tail_sizes || !g->tail_streams || !g->fsz)
        OPEN_FAIL("flake_amd_recode_set_open: out of host memory");
    return g;
#undef OPEN_FAIL
}

FLAKE_AMD_API int flake_amd_recode_set_enable_verify(FlakeAmdRecodeSet *g, int on)
{
    return g ? flake_amd_set_enable_verify(g->enc, on) : -1;
}

/* Seek points are the inner stream set's: it commits the new blocks. */
FLAKE_AMD_API int flake_amd_recode_set_seekpoints(FlakeAmdRecodeSet *g, unsigned long long spacing)
{
    return g ? flake_amd_set_seekpoints(g->enc, spacing) : -1;
}

FLAKE_AMD_API long long flake_amd_recode_set_get_seekpoints(const FlakeAmdRecodeSet *g, int stream, FlakeAmdSeekPoint *p, int cap)
{
    if (!g || stream < 0 || stream >= g->nstreams) return -1;
    if (g->st[stream].failed || flake_amd_decode_set_failed(g->dec, stream, NULL, NULL) == 1) return -1;
    return flake_amd_set_get_seekpoints(g->enc, stream, p, cap);
}

static long long rc_carry_total(const FlakeAmdRecodeSet *g)
{
    long long n = 0;
    for (int s = 0; s < g->nstreams; s++) n += g->st[s].carry_len;
    return n;
}

FLAKE_AMD_API int flake_amd_recode_set_out_bound(const FlakeAmdRecodeSet *g, long long nframes, size_t *bytes, long long *blocks)
{
    if (!g) return -1;
    long long nb;
    if (nframes < 0) {
        /* flake_amd_recode_set_finish: one short block per stream that holds a carry */
        nb = 0;
        for (int s = 0; s < g->nstreams; s++) nb += !g->st[s].failed && g->st[s].carry_len > 0;
    } else {
        nb = (rc_carry_total(g) + nframes * (long long)g->src_max_block) / g->block;
    }
    if (bytes) *bytes = (size_t)nb * (size_t)g->per_block;
    if (blocks) *blocks = nb;
    return 0;
}

/* One decode batch, judged by the decode set: its whole blocks are encoded behind the call's earlier ones and the
 * carries move to the other buffer. */
static int rc_batch(void *user, int nsegs, const int32_t *seg_stream, const int64_t *seg_start, const int64_t *seg_samples,
                    const unsigned char *seg_ok)
{
    FlakeAmdRecodeSet *g = (FlakeAmdRecodeSet *)user;
    const int room = g->block_cap - g->nblocks;
    const int nb = fa_rc_plan_batch(g->nstreams, g->st, g->block, nsegs, seg_stream, seg_start, seg_samples, seg_ok,
                                    room < g->plan_blocks ? room : g->plan_blocks, &g->plan);
    if (nb < 0) RC_FAIL("flake_amd_recode_set_frames: more blocks than the bound allows");       /* (cannot happen) */
    const int32_t *old_carry = g->d_carry[g->cur];
    if (nb > 0) {
        fa_set_source src = {g->plan.block_pieces, g->plan.nblock_pieces, old_carry, g->d_dec, (int64_t)g->carry_cap,
                             (int64_t)g->dec_cap, g->work, 0};
        const long long bytes = fa_set_encode_from(g->enc, &src, nb, g->block, g->plan.block_stream, g->out + g->out_at,
                                                   g->out_size - g->out_at, g->fsz);
        if (bytes < 0) RC_FAIL("%s", flake_amd_set_last_error(g->enc));
        for (int b = 0; b < nb; b++) {
            g->block_stream[g->nblocks + b] = g->plan.block_stream[b];
            g->block_bytes[g->nblocks + b] = g->fsz[b];
        }
        g->nblocks += nb;
        g->out_at += (size_t)bytes;
    }
    /* behind the block gathers on the same stream, and into the other buffer: nothing it reads is written */
    struct fhip_ctx *hip = fa_set_handle(g->enc);
    int rc = fhip_gather_spans_dev(hip, g->d_carry[g->cur ^ 1], (int64_t)g->carry_cap, old_carry, (int64_t)g->carry_cap,
                                   g->d_dec, (int64_t)g->dec_cap, g->plan.carry_pieces, g->plan.ncarry_pieces);
    if (rc == FHIP_OK) rc = fhip_sync(hip);                   /* the next decode batch overwrites d_dec */
    if (rc != FHIP_OK) RC_FAIL("fhip_gather_spans_dev: %s (%s)", fhip_strerror(rc), fhip_last_error(hip));
    g->cur ^= 1;
    return 0;
}

FLAKE_AMD_API long long flake_amd_recode_set_frames(FlakeAmdRecodeSet *g, int nruns, const int *stream_of_run,
                                                    const int *frames_of_run, const unsigned char *stream, size_t bytes,
                                                    const int *frame_sizes, unsigned char *out, size_t out_size,
                                                    int *block_stream, int *block_bytes, int block_cap, int *nblocks)
{
    if (!g) return -1;
    g->err[0] = 0;
    if (g->broken) RC_FAIL("flake_amd_recode_set_frames: an earlier device error left the set unusable");
    if (g->finished) RC_FAIL("flake_amd_recode_set_frames: the set has been finished: it takes no more frames");
    if (nruns < 0 || !nblocks || block_cap < 0 || (nruns > 0 && (!stream_of_run || !frames_of_run)))
        RC_FAIL("flake_amd_recode_set_frames: bad argument");
    long long nframes = 0;
    for (int r = 0; r < nruns; r++) {
        if (frames_of_run[r] < 0) RC_FAIL("flake_amd_recode_set_frames: bad argument");
        nframes += frames_of_run[r];
    }
    size_t need_bytes = 0;
    long long need_blocks = 0;
    (void)flake_amd_recode_set_out_bound(g, nframes, &need_bytes, &need_blocks);
    if (out_size < need_bytes || block_cap < need_blocks || (need_blocks > 0 && (!out || !block_stream || !block_bytes)))
        RC_FAIL("flake_amd_recode_set_frames: out_size %zu / block_cap %d are below the bound for %lld frames (%zu bytes, "
                "%lld blocks: flake_amd_recode_set_out_bound)", out_size, block_cap, nframes, need_bytes, need_blocks);
    if (nruns > g->run_cap) {
        long long *n = (long long *)realloc(g->run_samples, sizeof(long long) * (size_t)nruns);
        if (!n) RC_FAIL("flake_amd_recode_set_frames: out of host memory");
        g->run_samples = n;
        g->run_cap = nruns;
    }
    g->out = out; g->out_size = out_size; g->out_at = 0;
    g->block_stream = block_stream; g->block_bytes = block_bytes; g->block_cap = block_cap; g->nblocks = 0;
    *nblocks = 0;
    const long long batches0 = flake_amd_decode_set_device_batches(g->dec);
    const long long rc = fa_decode_set_frames_keep(g->dec, nruns, stream_of_run, frames_of_run, stream, bytes, frame_sizes,
                                                   g->d_dec, g->dec_cap, g->run_samples, rc_batch, g);
    if (rc < 0) {
        /* the decode set refuses a bad call before it changes anything; once a batch has run, the set is part way */
        if (flake_amd_decode_set_device_batches(g->dec) != batches0) g->broken = 1;
        if (!g->err[0]) snprintf(g->err, sizeof g->err, "%s", flake_amd_decode_set_last_error(g->dec));
        return -1;
    }
    *nblocks = g->nblocks;
    return (long long)g->out_at;
}

FLAKE_AMD_API long long flake_amd_recode_set_finish(FlakeAmdRecodeSet *g, unsigned char *out, size_t out_size,
                                                    int *block_stream, int *block_bytes, int block_cap, int *nblocks)
{
    if (!g) return -1;
    g->err[0] = 0;
    if (g->broken) RC_FAIL("flake_amd_recode_set_finish: an earlier device error left the set unusable");
    if (g->finished) RC_FAIL("flake_amd_recode_set_finish: the set has been finished already");
    if (!nblocks || block_cap < 0) RC_FAIL("flake_amd_recode_set_finish: bad argument");
    size_t need_bytes = 0;
    long long need_blocks = 0;
    (void)flake_amd_recode_set_out_bound(g, -1, &need_bytes, &need_blocks);
    if (out_size < need_bytes || block_cap < need_blocks || (need_blocks > 0 && (!out || !block_stream || !block_bytes)))
        RC_FAIL("flake_amd_recode_set_finish: out_size %zu / block_cap %d are below the bound (%zu bytes, %lld blocks: "
                "flake_amd_recode_set_out_bound with nframes -1)", out_size, block_cap, need_bytes, need_blocks);
    g->finished = 1;
    *nblocks = 0;
    /* every good stream's carry is its tail: one ragged call, one device batch per FLAKE_AMD_BATCH of them */
    int np = 0, next = 0;
    const int n = fa_rc_plan_tails(g->nstreams, g->st, 0, g->nstreams, g->plan.block_pieces, &np, g->tail_sizes,
                                   g->tail_streams, &next);
    if (n == 0) return 0;
    fa_set_source src = {g->plan.block_pieces, np, g->d_carry[g->cur], NULL, (int64_t)g->carry_cap, 0, g->work, 0};
    const long long bytes = fa_set_encode_short_from(g->enc, &src, n, g->tail_sizes, g->tail_streams, out, out_size, g->fsz);
    if (bytes < 0) { g->broken = 1; RC_FAIL("%s", flake_amd_set_last_error(g->enc)); }
    for (int b = 0; b < n; b++) {
        block_stream[b] = g->tail_streams[b];
        block_bytes[b] = g->fsz[b];
        g->st[g->tail_streams[b]].carry_len = 0;
    }
    *nblocks = n;
    return bytes;
}

FLAKE_AMD_API int flake_amd_recode_set_failed(const FlakeAmdRecodeSet *g, int stream, long long *frame, int *status)
{
    return g ? flake_amd_decode_set_failed(g->dec, stream, frame, status) : -1;
}

FLAKE_AMD_API int flake_amd_recode_set_get_streaminfo(FlakeAmdRecodeSet *g, int stream, FlakeAmdStreaminfo *si)
{
    if (!g || !si) return -1;
    g->err[0] = 0;
    if (stream < 0 || stream >= g->nstreams) RC_FAIL("flake_amd_recode_set_get_streaminfo: no stream %d in a set of %d", stream, g->nstreams);
    if (g->st[stream].failed || flake_amd_decode_set_failed(g->dec, stream, NULL, NULL) == 1)
        RC_FAIL("flake_amd_recode_set_get_streaminfo: stream %d has failed: it has no STREAMINFO", stream);
    if (flake_amd_set_get_streaminfo(g->enc, stream, si) != 0) RC_FAIL("%s", flake_amd_set_last_error(g->enc));
    /* the digest is the decode side's: the samples were hashed once, where K7 left them */
    if (!(g->flags & FLAKE_AMD_SET_MD5_OFF) && flake_amd_decode_set_md5(g->dec, stream, si->md5sum) != 0)
        RC_FAIL("%s", flake_amd_decode_set_last_error(g->dec));
    return 0;
}

FLAKE_AMD_API int flake_amd_recode_set_device_batches(const FlakeAmdRecodeSet *g, long long *decode, long long *encode)
{
    if (!g) return -1;
    if (decode) *decode = flake_amd_decode_set_device_batches(g->dec);
    if (encode) *encode = flake_amd_set_device_batches(g->enc);
    return 0;
}
