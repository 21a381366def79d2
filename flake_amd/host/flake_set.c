/*
 * flake_set.c -- the stream set of include/flake_amd.h: one batch path for many independent streams that share
 * their parameters (a library of files, not one long file).
 *
 * A batch is nblocks blocks back to back, block b belonging to stream stream_of_block[b].  The encode side needs
 * nothing new -- frames are independent and fhip_batch.frame_numbers numbers each one explicitly -- so the set keeps
 * what libflake keeps per stream (frame counter, sample count, min / max frame size, the last-block latch:
 * encode.c:967-992) and hands the batch to the packed path in chunks.  The MD5 (encode.c:1006, metadata.c:61-62) is
 * sequential inside a stream and independent across streams: each stream's running hash lives on the device (K6,
 * fhip_md5_state), updated from the PCM the chunk's upload has already brought there, beside the chunk's encode
 * kernels.  The samples cross the link once and the host hashes nothing.
 *
 * Verification (flake_amd_set_enable_verify) is the handle's own (fhip_set_verify): the packed path hands the chunk's
 * number table to the verifier, which holds every frame to its own stream's counter.  The verifier speaks of batch
 * indices; this file maps an index back to its stream and that stream's frame number.
 *
 * Variable block size (FLAKE_AMD_SET_VBS, levels 9-12): frames are numbered by their first sample, a block may become
 * several frames and a short block ends nothing (encode.c:993).  Blocks the splitter takes (a multiple of 8, at least
 * 128 samples: encode.c:997-999) go through fhip_encode_blocks_vbs_packed_numbered with each block's first-sample
 * number; every other length goes through the packed path as one frame per block, with fhip_set_block_numbering on.
 * The short blocks of a flake_amd_set_encode_ragged call -- splittable or not, each of its own length -- go through
 * fhip_encode_blocks_vbs_ragged_numbered, one device batch per FLAKE_AMD_BATCH of them.
 *
 * Encode rows (flake_amd_set_encode_rows): the samples are rows of a planar batch that already lies on the device.  The
 * call is planned into whole blocks and short blocks (rows_plan.h) and runs the two paths above with a source of row
 * pieces in place of a host buffer: each chunk's upload becomes fhip_frames_packed_from_rows (K12), nothing else changes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"
#include "flakehip.h"
#include "host_internal.h"
#include "recode_plan.h"
#include "rows_plan.h"
#include "seekpoints.h"

struct FlakeAmdSet {
    fhip_ctx *hip;
    fhip_params hp;
    int nstreams;
    unsigned flags;
    int max_batch;                        /* blocks per GPU batch (FLAKE_AMD_BATCH, default 1024) */
    int vbs;                              /* FLAKE_AMD_SET_VBS: frames numbered by sample, blocks may split */
    int pcm_format;
    int verbatim_size;                    /* of a full block: where max_frame_size starts (encode.c:446-450) */
    int broken;                           /* a device call failed half way: the streams' state is unknown */
    long long device_batches;             /* chunks handed to an encode entry of the HIP layer since the set was opened */
    int vfail, vfail_stream, vfail_status; /* flake_amd_set_last_verify_failure: the last encode call's, if any */
    unsigned vfail_number;
    /* per stream */
    uint32_t *frame_count;
    uint64_t *samples;
    int *min_frame, *max_frame;
    char *ended;
    int *scratch;                         /* [nstreams + 1] blocks per stream in a call / a chunk's CSR rows */
    fa_md5 *host_md5;                     /* FLAKE_AMD_SET_MD5_HOST */
    fa_seekrec *seek;                     /* flake_amd_set_seekpoints: one recorder per stream; null: off */
    flac_format seek_fmt;                 /* what a recorder reads a block's first header against */
    fhip_md5_state *dev_md5;              /* device memory */
    uint8_t *digests;                     /* [nstreams][16], fetched for all streams at once ... */
    int digests_valid;                    /* ... by the first request after an encode */
    /* per call, grown on demand */
    uint32_t *fnum;
    int32_t *fbytes;
    int32_t *seg_block;
    int32_t *bframes, *bmax;              /* variable block size: frames per block, each block's largest frame */
    int cap_blocks;
    char err[256];
};

static __thread char open_err[256];

FLAKE_AMD_API const char *flake_amd_set_last_error(const FlakeAmdSet *g) { return g ? g->err : open_err; }

FLAKE_AMD_API void flake_amd_set_close(FlakeAmdSet *g)
{
    if (!g) return;
    if (g->hip) {
        (void)fhip_sync(g->hip);
        (void)fhip_frames_packed_fetch_wait(g->hip);
        if (g->dev_md5) fhip_device_free(g->dev_md5);
        fhip_destroy(g->hip);
    }
    free(g->frame_count); free(g->samples); free(g->min_frame); free(g->max_frame); free(g->ended);
    free(g->scratch); free(g->host_md5); free(g->digests); free(g->fnum); free(g->fbytes); free(g->seg_block);
    free(g->bframes); free(g->bmax);
    if (g->seek) for (int s = 0; s < g->nstreams; s++) fa_seekrec_free(&g->seek[s]);
    free(g->seek);
    free(g);
}

FLAKE_AMD_API FlakeAmdSet *flake_amd_set_open(const FlakeAmdContext *like, int nstreams, unsigned flags)
{
    open_err[0] = 0;
#define OPEN_FAIL(...) do { snprintf(open_err, sizeof open_err, __VA_ARGS__); flake_amd_set_close(g); return NULL; } while (0)
    FlakeAmdSet *g = NULL;
    if (!like || flake_amd_validate_params(like) < 0) OPEN_FAIL("flake_amd_set_open: invalid parameters (flake_validate_params)");
    if (nstreams < 1) OPEN_FAIL("flake_amd_set_open: nstreams must be at least 1");
    if ((flags & ~(FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF | FLAKE_AMD_SET_VBS)) ||
        (flags & (FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF)) == (FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF))
        OPEN_FAIL("flake_amd_set_open: unknown or contradictory flags");
    if ((like->params.variable_block_size || like->params.allow_vbs) && !(flags & FLAKE_AMD_SET_VBS))
        OPEN_FAIL("flake_amd_set_open: variable block size (levels 9-12) is not supported for stream sets");
    if ((flags & FLAKE_AMD_SET_VBS) && !like->params.variable_block_size)
        OPEN_FAIL("flake_amd_set_open: FLAKE_AMD_SET_VBS needs parameters with variable block size (levels 9-12)");
    {
        const char *eha = getenv("FLAKE_AMD_HOST_ASSEMBLY"), *ehv = getenv("FLAKE_AMD_HOST_VBS");
        if ((eha && eha[0] == '1') || (ehv && ehv[0] == '1'))
            OPEN_FAIL("flake_amd_set_open: stream sets are not supported with FLAKE_AMD_HOST_ASSEMBLY / "
                      "FLAKE_AMD_HOST_VBS (CPU comparison modes)");
    }
    g = (FlakeAmdSet *)calloc(1, sizeof *g);
    if (!g) OPEN_FAIL("flake_amd_set_open: out of host memory");
    g->nstreams = nstreams;
    g->flags = flags;
    g->vbs = (flags & FLAKE_AMD_SET_VBS) != 0;
    fhip_params *hp = &g->hp;
    hp->channels = like->channels; hp->sample_rate = like->sample_rate;
    hp->bits_per_sample = like->bits_per_sample; hp->block_size = like->params.block_size;
    hp->order_method = like->params.order_method; hp->stereo_method = like->params.stereo_method;
    hp->prediction_type = like->params.prediction_type;
    hp->min_prediction_order = like->params.min_prediction_order;
    hp->max_prediction_order = like->params.max_prediction_order;
    hp->min_partition_order = like->params.min_partition_order;
    hp->max_partition_order = like->params.max_partition_order;
    hp->variable_block_size = g->vbs; hp->allow_vbs = g->vbs;        /* (validated: variable_block_size implies allow_vbs) */
    hp->lpc_precision = 15;                                       /* encode.c:443 */
    {
        const int bps = hp->bits_per_sample, n = hp->block_size;  /* encode.c:521-527 */
        g->verbatim_size = hp->channels == 2 ? 16 + ((n * (bps + bps + 1) + 7) >> 3)
                                             : 16 + ((n * hp->channels * bps + 7) >> 3);
    }
    const char *eb = getenv("FLAKE_AMD_BATCH"), *ed = getenv("FLAKE_AMD_DEVICE");
    g->max_batch = eb ? atoi(eb) : 1024;
    if (g->max_batch < 1) g->max_batch = 1;
    /* a block may become eight frames: the handle is sized as flake_amd_encode_init sizes it */
    const int rc = fhip_create(&g->hip, ed ? atoi(ed) : 0, hp, g->vbs ? g->max_batch * 8 : g->max_batch);
    if (rc != FHIP_OK) { g->hip = NULL; OPEN_FAIL("flake_amd_set_open: fhip_create: %s", fhip_strerror(rc)); }
    if (g->vbs && fhip_set_block_numbering(g->hip, 1) != FHIP_OK)
        OPEN_FAIL("flake_amd_set_open: fhip_set_block_numbering: %s", fhip_last_error(g->hip));
    const size_t ns = (size_t)nstreams;
    g->frame_count = (uint32_t *)calloc(ns, sizeof(uint32_t));
    g->samples = (uint64_t *)calloc(ns, sizeof(uint64_t));
    g->min_frame = (int *)calloc(ns, sizeof(int));
    g->max_frame = (int *)calloc(ns, sizeof(int));
    g->ended = (char *)calloc(ns, 1);
    g->scratch = (int *)calloc(ns + 1, sizeof(int));
    g->digests = (uint8_t *)calloc(ns, 16);
    if (!g->frame_count || !g->samples || !g->min_frame || !g->max_frame || !g->ended || !g->scratch || !g->digests)
        OPEN_FAIL("flake_amd_set_open: out of host memory");
    for (int s = 0; s < nstreams; s++) g->max_frame[s] = g->verbatim_size;
    if (flags & FLAKE_AMD_SET_MD5_HOST) {
        g->host_md5 = (fa_md5 *)calloc(ns, sizeof(fa_md5));
        if (!g->host_md5) OPEN_FAIL("flake_amd_set_open: out of host memory");
        for (int s = 0; s < nstreams; s++) fa_md5_init(&g->host_md5[s]);
    } else if (!(flags & FLAKE_AMD_SET_MD5_OFF)) {
        g->dev_md5 = (fhip_md5_state *)fhip_device_alloc(ns * sizeof(fhip_md5_state));
        if (!g->dev_md5) OPEN_FAIL("flake_amd_set_open: no device memory for %d MD5 states", nstreams);
        const int r2 = fhip_md5_init_dev(g->hip, g->dev_md5, nstreams);
        if (r2 != FHIP_OK) OPEN_FAIL("flake_amd_set_open: fhip_md5_init_dev: %s (%s)", fhip_strerror(r2), fhip_last_error(g->hip));
    }
    g->digests_valid = 1;                 /* of the empty message, or zeros: set below / on request */
    if (g->dev_md5) g->digests_valid = 0;
    if (g->host_md5) for (int s = 0; s < nstreams; s++) fa_md5_final(&g->host_md5[s], g->digests + 16 * (size_t)s);
    return g;
#undef OPEN_FAIL
}

FLAKE_AMD_API long long flake_amd_set_device_batches(const FlakeAmdSet *g) { return g ? g->device_batches : -1; }

FLAKE_AMD_API int flake_amd_set_enable_verify(FlakeAmdSet *g, int on)
{
    if (!g) return -1;
    return fhip_set_verify(g->hip, on != 0) == FHIP_OK ? 0 : -1;
}

FLAKE_AMD_API int flake_amd_set_last_verify_failure(const FlakeAmdSet *g, int *stream, unsigned *frame_number, int *status)
{
    if (!g || !g->vfail) return 0;
    if (stream) *stream = g->vfail_stream;
    if (frame_number) *frame_number = g->vfail_number;
    if (status) *status = g->vfail_status;
    return 1;
}

static const char *verify_status_name(int s)
{
    static const char *const names[] = {"OK", "HEADER", "CRC8", "NUMBER", "SYNTAX", "SAMPLES", "PADDING", "CRC16", "LENGTH"};
    return (s >= 0 && s <= 8) ? names[s] : "?";
}

static int grow_call_tables(FlakeAmdSet *g, int nblocks)
{
    if (nblocks <= g->cap_blocks) return 0;
    free(g->fnum); free(g->fbytes); free(g->seg_block); free(g->bframes); free(g->bmax);
    g->bframes = g->bmax = NULL;
    g->cap_blocks = 0;
    g->fnum = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)nblocks);
    g->fbytes = (int32_t *)malloc(sizeof(int32_t) * (size_t)nblocks);
    g->seg_block = (int32_t *)malloc(sizeof(int32_t) * (size_t)nblocks);
    if (!g->fnum || !g->fbytes || !g->seg_block) return -1;
    if (g->vbs) {
        g->bframes = (int32_t *)malloc(sizeof(int32_t) * (size_t)nblocks);
        g->bmax = (int32_t *)malloc(sizeof(int32_t) * (size_t)nblocks);
        if (!g->bframes || !g->bmax) return -1;
    }
    g->cap_blocks = nblocks;
    return 0;
}

#define SET_FAIL(...) do { snprintf(g->err, sizeof g->err, __VA_ARGS__); return -1; } while (0)

/* A chunk (blocks b0 .. b0 + cnt of the call) came back FHIP_E_VERIFY from the entry `what`: the verifier's first
 * failing frame is an index into the chunk; name its block, from there its stream, and the number it had to carry.
 * block_frames: the chunk's frames per block where blocks were split (numbered by first sample), null for one frame
 * per block; ragged: flake_amd_set_encode_ragged's call.  Nothing of the call is committed, the device hashes have
 * moved on.  Returns -1 with the set's error text and vfail fields filled. */
static long long set_verify_failed(FlakeAmdSet *g, const char *what, const int *stream_of_block, int b0, int cnt,
                                   const int32_t *block_frames, int ragged)
{
    int64_t vs[4] = {0, 0, -1, 0};
    fhip_verify_rec vr = {0, -1, -1, -1};
    uint32_t number = 0;
    (void)fhip_last_verify_failure(g->hip, vs, &vr);
    const int have_number = fhip_last_verify_number(g->hip, &number) == 1;
    g->broken = g->dev_md5 != NULL;
    const int blk = fa_block_of_frame(vs[2], block_frames, cnt);
    if (blk < 0) SET_FAIL("%s: %s (%s)", what, fhip_strerror(FHIP_E_VERIFY), fhip_last_error(g->hip));
    const int idx = b0 + blk;
    g->vfail = 1;
    g->vfail_stream = stream_of_block[idx];
    g->vfail_number = have_number ? number : g->fnum[idx];      /* (the frame's own; unplaceable: the block's first) */
    g->vfail_status = vr.status;
    SET_FAIL("flake_amd_set_encode%s: verification failed: %lld of the chunk's %lld frames do not decode to the "
             "input; first: stream %d, %s %u (%sblock %d of the call), %s (subframe %d, sample %d, bit %d)",
             ragged ? "_ragged" : "", (long long)vs[1], (long long)vs[0], g->vfail_stream,
             block_frames ? "first sample" : "frame", g->vfail_number, ragged ? "short " : "", idx,
             verify_status_name(vr.status), vr.subframe, vr.sample, vr.bit);
}

/* The upload step of a chunk, or its stand-in for a call whose samples are gather pieces or row pieces (fa_set_source):
 * the chunk is samples lo .. hi of the call; bt->pcm is then a token that names the batch. */
static int set_bring(FlakeAmdSet *g, fa_set_source *src, const fhip_batch *bt, const int32_t *sizes, long long lo,
                     long long hi, const char **what)
{
    if (!src) {
        *what = sizes ? "fhip_frames_packed_upload_ragged" : "fhip_frames_packed_upload";
        return sizes ? fhip_frames_packed_upload_ragged(g->hip, bt, sizes) : fhip_frames_packed_upload(g->hip, bt);
    }
    if (src->rows) {
        *what = "fhip_frames_packed_from_rows";
        const int k = fa_rows_slice(src->row_pieces, src->npieces, &src->cur, lo, hi, src->row_work);
        return fhip_frames_packed_from_rows(g->hip, bt, sizes, src->rows, src->row_work, k);
    }
    *what = "fhip_frames_packed_gather";
    const int m = fa_rc_slice(src->pieces, src->npieces, &src->cur, lo, hi, src->work);
    return fhip_frames_packed_gather(g->hip, bt, sizes, src->src0, src->src0_cap, src->src1, src->src1_cap, src->work, m);
}

static long long set_encode(FlakeAmdSet *g, fa_set_source *src, const void *samples, int sample_bytes, int nblocks,
                            int block_size, const int *stream_of_block, unsigned char *out, size_t out_size,
                            int *frame_sizes)
{
    if (!g) return -1;
    g->err[0] = 0;
    g->vfail = 0;
    if (g->broken) SET_FAIL("flake_amd_set_encode: an earlier device error left the set unusable");
    if (nblocks < 0 || (nblocks > 0 && (!samples || !stream_of_block || !out)))
        SET_FAIL("flake_amd_set_encode: null argument or negative block count");
    if (sample_bytes != 4 && sample_bytes != 2) SET_FAIL("flake_amd_set_encode: sample_bytes must be 4 or 2");
    if (sample_bytes == 2 && g->hp.bits_per_sample > 16)
        SET_FAIL("flake_amd_set_encode: int16 samples need bits_per_sample <= 16");
    if (sample_bytes == 2 && g->vbs)
        SET_FAIL("flake_amd_set_encode: int16 samples are not supported with variable block size (levels 9-12)");
    if (block_size < 1 || block_size > g->hp.block_size)
        SET_FAIL("flake_amd_set_encode: block_size out of range (encode.c:987)");
    if (nblocks == 0) return 0;
    /* everything is checked before anything changes: the streams exist, none has ended (encode.c:989), and a
     * short block -- which ends its stream (encode.c:991-992) -- is its stream's only block of the call */
    const int is_short = !g->vbs && block_size != g->hp.block_size;       /* (allow_vbs: no latch, encode.c:993) */
    /* the blocks split_frame_v1 sees (encode.c:997-999); any other length is one frame per block */
    const int split = g->vbs && (block_size % 8) == 0 && block_size >= 128;
    int *per = g->scratch;
    memset(per, 0, sizeof(int) * (size_t)g->nstreams);
    for (int b = 0; b < nblocks; b++) {
        const int s = stream_of_block[b];
        if (s < 0 || s >= g->nstreams) SET_FAIL("flake_amd_set_encode: stream_of_block[%d] = %d is outside the set's %d streams", b, s, g->nstreams);
        if (g->ended[s] || (is_short && per[s]))
            SET_FAIL("flake_amd_set_encode: block %d belongs to stream %d, which a short block has ended", b, s);
        per[s]++;
    }
    if (grow_call_tables(g, nblocks)) SET_FAIL("flake_amd_set_encode: out of host memory");
    const int fmt = sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32;
    if (fmt != g->pcm_format) {
        const int rc = fhip_set_pcm_format(g->hip, fmt);
        if (rc != FHIP_OK) SET_FAIL("fhip_set_pcm_format: %s (%s)", fhip_strerror(rc), fhip_last_error(g->hip));
        g->pcm_format = fmt;
    }
    /* frame numbers: each stream counts its own frames -- its own samples with allow_vbs (encode.c:969-975) */
    memset(per, 0, sizeof(int) * (size_t)g->nstreams);
    for (int b = 0; b < nblocks; b++) {
        const int s = stream_of_block[b];
        g->fnum[b] = g->frame_count[s] + (uint32_t)per[s]++ * (g->vbs ? (uint32_t)block_size : 1u);
    }
    const size_t bstride = (size_t)block_size * (size_t)g->hp.channels * (size_t)sample_bytes;
    long long total = 0;
    int rc = FHIP_OK;
    const char *what = "";
    for (int b0 = 0; b0 < nblocks && rc == FHIP_OK; b0 += g->max_batch) {
        const int cnt = nblocks - b0 < g->max_batch ? nblocks - b0 : g->max_batch;
        fhip_batch bt;
        memset(&bt, 0, sizeof bt);
        bt.pcm = (const int32_t *)((const char *)samples + (size_t)b0 * bstride);
        bt.nframes = cnt; bt.block_size = block_size;
        bt.frame_bytes = g->fbytes + b0;
        bt.frame_numbers = g->fnum + b0;
        rc = set_bring(g, src, &bt, NULL, (long long)b0 * block_size, (long long)(b0 + cnt) * block_size, &what);
        if (rc == FHIP_OK && g->dev_md5) {
            /* the chunk's blocks per stream, in batch order (CSR), for the hash that runs beside the encode kernels */
            int *first = g->scratch;
            memset(first, 0, sizeof(int) * ((size_t)g->nstreams + 1));
            for (int b = 0; b < cnt; b++) first[stream_of_block[b0 + b] + 1]++;
            for (int s = 0; s < g->nstreams; s++) first[s + 1] += first[s];
            for (int b = 0; b < cnt; b++) g->seg_block[first[stream_of_block[b0 + b]]++] = b;
            for (int s = g->nstreams; s > 0; s--) first[s] = first[s - 1];      /* the fill moved every row's start up */
            first[0] = 0;
            what = "fhip_md5_update_uploaded";
            rc = fhip_md5_update_uploaded(g->hip, g->dev_md5, g->nstreams, cnt, block_size, (const int32_t *)first, g->seg_block);
        }
        int64_t bytes = 0;
        if (rc == FHIP_OK) g->device_batches++;
        if (rc == FHIP_OK && split) {
            /* split, encoded and packed on the device, block b numbered from its stream's sample count; the bytes
             * come back before the call returns (no download beside the next chunk's upload on this path) */
            what = "fhip_encode_blocks_vbs_packed_numbered";
            rc = fhip_encode_blocks_vbs_packed_numbered(g->hip, bt.pcm, cnt, block_size, g->fnum + b0, out + total,
                                                        (int64_t)(out_size - (size_t)total), g->fbytes + b0,
                                                        g->bframes + b0, g->bmax + b0, &bytes);
            /* (the verifier's frame index counts the chunk's FRAMES: block_frames says which block it lies in) */
            if (rc == FHIP_E_VERIFY) return set_verify_failed(g, what, stream_of_block, b0, cnt, g->bframes + b0, 0);
            if (rc == FHIP_OK) total += bytes;
            continue;
        }
        if (rc == FHIP_OK) { what = "fhip_frames_packed_begin"; rc = fhip_frames_packed_begin(g->hip, &bt, &bytes); }
        if (rc == FHIP_E_VERIFY) {
            (void)fhip_frames_packed_fetch_wait(g->hip);
            return set_verify_failed(g, what, stream_of_block, b0, cnt, NULL, 0);
        }
        if (rc == FHIP_OK && (size_t)(total + bytes) > out_size) {
            (void)fhip_frames_packed_fetch_wait(g->hip);
            g->broken = g->dev_md5 != NULL;          /* (its hashes have moved on) */
            SET_FAIL("flake_amd_set_encode: output buffer too small (%lld bytes needed so far, %zu given)",
                     total + (long long)bytes, out_size);
        }
        /* (not waited for here: the download runs beside the next chunk's upload) */
        if (rc == FHIP_OK) { what = "fhip_frames_packed_fetch_async"; rc = fhip_frames_packed_fetch_async(g->hip, out + total, (int64_t)(out_size - (size_t)total)); }
        if (rc == FHIP_OK) total += bytes;
    }
    const int rcw = fhip_frames_packed_fetch_wait(g->hip);
    if (rc == FHIP_OK && rcw != FHIP_OK) { rc = rcw; what = "fhip_frames_packed_fetch_wait"; }
    if (rc != FHIP_OK) {
        g->broken = 1;
        SET_FAIL("%s: %s (%s)", what, fhip_strerror(rc), fhip_last_error(g->hip));
    }
    for (int b = 0; b < nblocks; b++)
        if (g->fbytes[b] <= 0) { g->broken = 1; SET_FAIL("flake_amd_set_encode: frame %d was not encoded", b); }
    /* the batch is part of its streams now */
    const size_t nvals = (size_t)block_size * (size_t)g->hp.channels;
    size_t at = 0;                         /* block b's first frame in out */
    for (int b = 0; b < nblocks; b++) {
        const int s = stream_of_block[b], fs = g->fbytes[b];
        if (g->seek && fa_seekrec_block_at(&g->seek[s], &g->seek_fmt, out + at, (unsigned long long)block_size, (unsigned long long)fs)) {
            g->broken = 1;
            SET_FAIL("flake_amd_set_encode: the seek point of block %d could not be recorded", b);
        }
        at += (size_t)fs;
        if (frame_sizes) frame_sizes[b] = fs;
        const int largest = split ? g->bmax[b] : fs;                        /* of the block's frames */
        if (largest > g->max_frame[s]) g->max_frame[s] = largest;           /* encode.c:967 */
        if (!g->min_frame[s] || fs < g->min_frame[s]) g->min_frame[s] = fs;
        g->frame_count[s] += g->vbs ? (uint32_t)block_size : 1u;            /* encode.c:969-975 */
        g->samples[s] += (uint64_t)block_size;
        if (is_short) g->ended[s] = 1;
        if (g->host_md5) {
            const char *p = (const char *)samples + (size_t)b * bstride;
            if (sample_bytes == 2) fa_md5_pcm16(&g->host_md5[s], (const int16_t *)p, nvals, g->hp.bits_per_sample);
            else fa_md5_pcm(&g->host_md5[s], (const int32_t *)p, nvals, g->hp.bits_per_sample);
        }
    }
    if (g->host_md5) for (int s = 0; s < g->nstreams; s++) fa_md5_final(&g->host_md5[s], g->digests + 16 * (size_t)s);
    if (g->dev_md5) g->digests_valid = 0;
    return total;
}

FLAKE_AMD_API long long flake_amd_set_encode(FlakeAmdSet *g, const void *samples, int sample_bytes, int nblocks,
                                             int block_size, const int *stream_of_block, unsigned char *out,
                                             size_t out_size, int *frame_sizes)
{
    return set_encode(g, NULL, samples, sample_bytes, nblocks, block_size, stream_of_block, out, out_size, frame_sizes);
}

/* The short blocks of a call through the ragged packed path: cnt blocks back to back, block b sizes[b] samples long
 * (every one shorter than the set's block size, one per stream: the caller has checked).  The twin of the loop in
 * flake_amd_set_encode.  With variable block size the chunk goes through fhip_encode_blocks_vbs_ragged_numbered
 * instead: a block may become several frames, is numbered from its stream's sample count and ends nothing
 * (encode.c:993); the bytes come back before the call returns, as on that path of flake_amd_set_encode.  Returns the bytes written, -1 on an error, or -2 when the ABI does not cover this handle
 * (FHIP_E_UNSUPPORTED on the first chunk: nothing has changed, the caller takes the per-length calls). */
static long long set_encode_short(FlakeAmdSet *g, fa_set_source *src, const void *samples, int sample_bytes, int cnt_all,
                                  const int *sizes, const int *stream_of_block, unsigned char *out, size_t out_size,
                                  int *frame_sizes)
{
    long long done_samples = 0;           /* of the chunks before this one */
    if (grow_call_tables(g, cnt_all)) SET_FAIL("flake_amd_set_encode_ragged: out of host memory");
    const int fmt = sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32;
    if (fmt != g->pcm_format) {
        const int rc = fhip_set_pcm_format(g->hip, fmt);
        if (rc != FHIP_OK) SET_FAIL("fhip_set_pcm_format: %s (%s)", fhip_strerror(rc), fhip_last_error(g->hip));
        g->pcm_format = fmt;
    }
    for (int b = 0; b < cnt_all; b++) g->fnum[b] = g->frame_count[stream_of_block[b]];      /* one block per stream */
    const size_t vbytes = (size_t)g->hp.channels * (size_t)sample_bytes;
    const char *pcm = (const char *)samples;
    long long total = 0;
    int rc = FHIP_OK;
    const char *what = "";
    for (int b0 = 0; b0 < cnt_all && rc == FHIP_OK; b0 += g->max_batch) {
        const int cnt = cnt_all - b0 < g->max_batch ? cnt_all - b0 : g->max_batch;
        size_t chunk_samples = 0;
        int largest = 0;
        for (int b = 0; b < cnt; b++) {
            chunk_samples += (size_t)sizes[b0 + b];
            if (sizes[b0 + b] > largest) largest = sizes[b0 + b];
        }
        fhip_batch bt;
        memset(&bt, 0, sizeof bt);
        bt.pcm = (const int32_t *)pcm;
        bt.nframes = cnt; bt.block_size = largest;
        bt.frame_bytes = g->fbytes + b0;
        bt.frame_numbers = g->fnum + b0;
        rc = set_bring(g, src, &bt, (const int32_t *)(sizes + b0), done_samples, done_samples + (long long)chunk_samples, &what);
        done_samples += (long long)chunk_samples;
        if (rc == FHIP_E_UNSUPPORTED && b0 == 0) return -2;
        if (rc == FHIP_OK && g->dev_md5) {
            int *first = g->scratch;
            memset(first, 0, sizeof(int) * ((size_t)g->nstreams + 1));
            for (int b = 0; b < cnt; b++) first[stream_of_block[b0 + b] + 1]++;
            for (int s = 0; s < g->nstreams; s++) first[s + 1] += first[s];
            for (int b = 0; b < cnt; b++) g->seg_block[first[stream_of_block[b0 + b]]++] = b;
            for (int s = g->nstreams; s > 0; s--) first[s] = first[s - 1];
            first[0] = 0;
            what = "fhip_md5_update_uploaded_ragged";
            rc = fhip_md5_update_uploaded_ragged(g->hip, g->dev_md5, g->nstreams, cnt, (const int32_t *)(sizes + b0),
                                                 (const int32_t *)first, g->seg_block);
        }
        int64_t bytes = 0;
        if (rc == FHIP_OK) g->device_batches++;
        if (rc == FHIP_OK && g->vbs) {
            what = "fhip_encode_blocks_vbs_ragged_numbered";
            rc = fhip_encode_blocks_vbs_ragged_numbered(g->hip, bt.pcm, cnt, (const int32_t *)(sizes + b0), g->fnum + b0,
                                                        out + total, (int64_t)(out_size - (size_t)total), g->fbytes + b0,
                                                        g->bframes + b0, g->bmax + b0, &bytes);
            /* (the verifier's frame index counts the chunk's FRAMES: block_frames says which block it lies in) */
            if (rc == FHIP_E_VERIFY) return set_verify_failed(g, what, stream_of_block, b0, cnt, g->bframes + b0, 1);
            if (rc == FHIP_OK) total += bytes;
            pcm += chunk_samples * vbytes;
            continue;
        }
        if (rc == FHIP_OK) {
            what = "fhip_frames_packed_begin_ragged";
            rc = fhip_frames_packed_begin_ragged(g->hip, &bt, (const int32_t *)(sizes + b0), &bytes);
        }
        if (rc == FHIP_E_VERIFY) {
            (void)fhip_frames_packed_fetch_wait(g->hip);
            return set_verify_failed(g, what, stream_of_block, b0, cnt, NULL, 1);
        }
        if (rc == FHIP_OK && (size_t)(total + bytes) > out_size) {
            (void)fhip_frames_packed_fetch_wait(g->hip);
            g->broken = g->dev_md5 != NULL;
            SET_FAIL("flake_amd_set_encode_ragged: output buffer too small (%lld bytes needed so far, %zu given)",
                     total + (long long)bytes, out_size);
        }
        if (rc == FHIP_OK) { what = "fhip_frames_packed_fetch_async"; rc = fhip_frames_packed_fetch_async(g->hip, out + total, (int64_t)(out_size - (size_t)total)); }
        if (rc == FHIP_OK) total += bytes;
        pcm += chunk_samples * vbytes;
    }
    const int rcw = fhip_frames_packed_fetch_wait(g->hip);
    if (rc == FHIP_OK && rcw != FHIP_OK) { rc = rcw; what = "fhip_frames_packed_fetch_wait"; }
    if (rc != FHIP_OK) {
        g->broken = 1;
        SET_FAIL("%s: %s (%s)", what, fhip_strerror(rc), fhip_last_error(g->hip));
    }
    for (int b = 0; b < cnt_all; b++)
        if (g->fbytes[b] <= 0) { g->broken = 1; SET_FAIL("flake_amd_set_encode_ragged: frame %d was not encoded", b); }
    pcm = (const char *)samples;
    size_t at = 0;                         /* block b's first frame in out */
    for (int b = 0; b < cnt_all; b++) {
        const int s = stream_of_block[b], fs = g->fbytes[b];
        const size_t nvals = (size_t)sizes[b] * (size_t)g->hp.channels;
        if (g->seek && fa_seekrec_block_at(&g->seek[s], &g->seek_fmt, out + at, (unsigned long long)sizes[b], (unsigned long long)fs)) {
            g->broken = 1;
            SET_FAIL("flake_amd_set_encode_ragged: the seek point of block %d could not be recorded", b);
        }
        at += (size_t)fs;
        if (frame_sizes) frame_sizes[b] = fs;
        const int largest = g->vbs ? g->bmax[b] : fs;                       /* of the block's frames */
        if (largest > g->max_frame[s]) g->max_frame[s] = largest;           /* encode.c:967 */
        if (!g->min_frame[s] || fs < g->min_frame[s]) g->min_frame[s] = fs;
        g->frame_count[s] += g->vbs ? (uint32_t)sizes[b] : 1u;              /* encode.c:969-975 */
        g->samples[s] += (uint64_t)sizes[b];
        if (!g->vbs) g->ended[s] = 1;                                       /* (allow_vbs: no latch, encode.c:993) */
        if (g->host_md5) {
            if (sample_bytes == 2) fa_md5_pcm16(&g->host_md5[s], (const int16_t *)pcm, nvals, g->hp.bits_per_sample);
            else fa_md5_pcm(&g->host_md5[s], (const int32_t *)pcm, nvals, g->hp.bits_per_sample);
        }
        pcm += nvals * (size_t)sample_bytes;
    }
    if (g->host_md5) for (int s = 0; s < g->nstreams; s++) fa_md5_final(&g->host_md5[s], g->digests + 16 * (size_t)s);
    if (g->dev_md5) g->digests_valid = 0;
    return total;
}

/* Blocks of different lengths in one call.  The blocks are sorted into groups that one device path serves -- the
 * full-length blocks (flake_amd_set_encode), the short ones (one ragged call; under FLAKE_AMD_SET_RAGGED=0, or where
 * the ABI does not cover the handle, one uniform call per distinct length) -- each group is gathered, encoded and its
 * frames put back in batch order.  A call that is a single group runs in place. */
FLAKE_AMD_API long long flake_amd_set_encode_ragged(FlakeAmdSet *g, const void *samples, int sample_bytes, int nblocks,
                                                    const int *block_sizes, const int *stream_of_block,
                                                    unsigned char *out, size_t out_size, int *frame_sizes)
{
    if (!g) return -1;
    g->err[0] = 0;
    g->vfail = 0;
    if (g->broken) SET_FAIL("flake_amd_set_encode_ragged: an earlier device error left the set unusable");
    if (nblocks < 0 || (nblocks > 0 && (!samples || !block_sizes || !stream_of_block || !out)))
        SET_FAIL("flake_amd_set_encode_ragged: null argument or negative block count");
    if (sample_bytes != 4 && sample_bytes != 2) SET_FAIL("flake_amd_set_encode_ragged: sample_bytes must be 4 or 2");
    if (sample_bytes == 2 && g->hp.bits_per_sample > 16)
        SET_FAIL("flake_amd_set_encode_ragged: int16 samples need bits_per_sample <= 16");
    if (sample_bytes == 2 && g->vbs)
        SET_FAIL("flake_amd_set_encode_ragged: int16 samples are not supported with variable block size (levels 9-12)");
    if (nblocks == 0) return 0;
    /* everything is checked before anything changes */
    const int full = g->hp.block_size;
    int *per = g->scratch;                /* 1: the stream has a short block in this call */
    memset(per, 0, sizeof(int) * (size_t)g->nstreams);
    int nshort = 0;
    for (int b = 0; b < nblocks; b++) {
        const int s = stream_of_block[b], n = block_sizes[b];
        if (n < 1 || n > full) SET_FAIL("flake_amd_set_encode_ragged: block_sizes[%d] = %d is out of range (encode.c:987)", b, n);
        if (s < 0 || s >= g->nstreams) SET_FAIL("flake_amd_set_encode_ragged: stream_of_block[%d] = %d is outside the set's %d streams", b, s, g->nstreams);
        if (g->ended[s] || per[s])
            SET_FAIL("flake_amd_set_encode_ragged: block %d belongs to stream %d, which a short block has ended", b, s);
        if (n != full) { per[s] = 1; nshort++; }
    }
    if (nshort == 0)
        return flake_amd_set_encode(g, samples, sample_bytes, nblocks, full, stream_of_block, out, out_size, frame_sizes);
    const char *er = getenv("FLAKE_AMD_SET_RAGGED");
    int ragged = !(er && er[0] == '0');
    if (ragged && nshort == nblocks) {
        const long long r = set_encode_short(g, NULL, samples, sample_bytes, nblocks, block_sizes, stream_of_block, out, out_size, frame_sizes);
        if (r != -2) return r;
        ragged = 0;
    }
    /* groups: gid[b] = 0 for a full block, 1 for every short one (ragged) or 1 + k for the k-th distinct length */
    const size_t vbytes = (size_t)g->hp.channels * (size_t)sample_bytes;
    size_t all_samples = 0;
    for (int b = 0; b < nblocks; b++) all_samples += (size_t)block_sizes[b];
    int *gid = (int *)malloc(sizeof(int) * (size_t)nblocks * 6);
    size_t *off = (size_t *)malloc(sizeof(size_t) * (size_t)nblocks * 2);
    char *gpcm = (char *)malloc(all_samples * vbytes);
    unsigned char *stash = (unsigned char *)malloc(out_size ? out_size : 1);
    const size_t ns = (size_t)g->nstreams;
    /* the streams as they are, put back if a later group fails */
    uint32_t *sv_fc = (uint32_t *)malloc(ns * sizeof(uint32_t));
    uint64_t *sv_sm = (uint64_t *)malloc(ns * sizeof(uint64_t));
    int *sv_mm = (int *)malloc(ns * 2 * sizeof(int));
    char *sv_en = (char *)malloc(ns);
    fa_md5 *sv_md = g->host_md5 ? (fa_md5 *)malloc(ns * sizeof(fa_md5)) : NULL;
    fa_seekrec_mark *sv_sk = g->seek ? (fa_seekrec_mark *)malloc(ns * sizeof(fa_seekrec_mark)) : NULL;
    long long result = -1;
#define RAGGED_DONE() do { free(gid); free(off); free(gpcm); free(stash); free(sv_fc); free(sv_sm); free(sv_mm); free(sv_en); free(sv_md); free(sv_sk); } while (0)
    if (!gid || !off || !gpcm || !stash || !sv_fc || !sv_sm || !sv_mm || !sv_en || (g->host_md5 && !sv_md) || (g->seek && !sv_sk)) {
        RAGGED_DONE();
        SET_FAIL("flake_amd_set_encode_ragged: out of host memory");
    }
    int *members = gid + nblocks, *gsizes = gid + 2 * nblocks, *gstreams = gid + 3 * nblocks;
    int *gfs = gid + 4 * nblocks, *fsz = gid + 5 * nblocks;      /* frame sizes: of the group's members / by block */
    size_t *src = off + nblocks;          /* byte offset of block b in samples */
    {
        size_t at = 0;
        for (int b = 0; b < nblocks; b++) { src[b] = at; at += (size_t)block_sizes[b] * vbytes; }
    }
    int ngroups = 1;                       /* group 0 may be empty */
    for (int b = 0; b < nblocks; b++) {
        if (block_sizes[b] == full) { gid[b] = 0; continue; }
        if (ragged) { gid[b] = 1; ngroups = 2; continue; }
        gid[b] = -1;
        for (int a = 0; a < b; a++) if (block_sizes[a] == block_sizes[b]) { gid[b] = gid[a]; break; }
        if (gid[b] < 0) gid[b] = ngroups++;
    }
    memcpy(sv_fc, g->frame_count, ns * sizeof(uint32_t)); memcpy(sv_sm, g->samples, ns * sizeof(uint64_t));
    memcpy(sv_mm, g->min_frame, ns * sizeof(int)); memcpy(sv_mm + ns, g->max_frame, ns * sizeof(int));
    memcpy(sv_en, g->ended, ns);
    if (sv_md) memcpy(sv_md, g->host_md5, ns * sizeof(fa_md5));
    if (sv_sk) for (int s = 0; s < g->nstreams; s++) sv_sk[s] = fa_seekrec_save(&g->seek[s]);
    size_t stash_at = 0;
    int ok = 1;
    for (int k = 0; k < ngroups && ok; k++) {
        int cnt = 0;
        size_t at = 0;
        for (int b = 0; b < nblocks; b++) {
            if (gid[b] != k) continue;
            const size_t bytes = (size_t)block_sizes[b] * vbytes;
            memcpy(gpcm + at, (const char *)samples + src[b], bytes);
            at += bytes;
            members[cnt] = b; gsizes[cnt] = block_sizes[b]; gstreams[cnt] = stream_of_block[b];
            cnt++;
        }
        if (cnt == 0) continue;
        long long r;
        if (k == 1 && ragged) {
            r = set_encode_short(g, NULL, gpcm, sample_bytes, cnt, gsizes, gstreams, stash + stash_at, out_size - stash_at, gfs);
            if (r == -2) {
                /* the ABI does not cover this handle: nothing of the short blocks has run; take the per-length calls */
                ragged = 0;
                ngroups = 1;
                for (int b = 0; b < nblocks; b++) {
                    if (gid[b] == 0) continue;
                    gid[b] = -1;
                    for (int a = 0; a < b; a++) if (gid[a] > 0 && block_sizes[a] == block_sizes[b]) { gid[b] = gid[a]; break; }
                    if (gid[b] < 0) gid[b] = ngroups++;
                }
                k = 0;                     /* (the loop's k++ makes it 1: group 0 is done) */
                continue;
            }
        } else {
            r = flake_amd_set_encode(g, gpcm, sample_bytes, cnt, gsizes[0], gstreams, stash + stash_at, out_size - stash_at, gfs);
        }
        if (r < 0) { ok = 0; break; }
        /* where each member's frame lies in the stash */
        size_t fat = stash_at;
        for (int i = 0; i < cnt; i++) {
            off[members[i]] = fat;
            fsz[members[i]] = gfs[i];
            fat += (size_t)gfs[i];
        }
        stash_at += (size_t)r;
    }
    if (!ok) {
        /* a group failed: its inner call has said why and committed nothing; the groups before it are taken back */
        memcpy(g->frame_count, sv_fc, ns * sizeof(uint32_t)); memcpy(g->samples, sv_sm, ns * sizeof(uint64_t));
        memcpy(g->min_frame, sv_mm, ns * sizeof(int)); memcpy(g->max_frame, sv_mm + ns, ns * sizeof(int));
        memcpy(g->ended, sv_en, ns);
        if (sv_sk) for (int s = 0; s < g->nstreams; s++) fa_seekrec_restore(&g->seek[s], &sv_sk[s]);
        if (sv_md) {
            memcpy(g->host_md5, sv_md, ns * sizeof(fa_md5));
            for (int s = 0; s < g->nstreams; s++) fa_md5_final(&g->host_md5[s], g->digests + 16 * (size_t)s);
        }
        if (g->dev_md5 && stash_at > 0) g->broken = 1;     /* (the device hashes of the earlier groups have moved on) */
        RAGGED_DONE();
        return -1;
    }
    {
        size_t at = 0;
        for (int b = 0; b < nblocks; b++) {
            memcpy(out + at, stash + off[b], (size_t)fsz[b]);
            if (frame_sizes) frame_sizes[b] = fsz[b];
            at += (size_t)fsz[b];
        }
        result = (long long)at;
    }
    RAGGED_DONE();
#undef RAGGED_DONE
    return result;
}

/* ---- the hooks of a recode set (host_internal.h) ---- */

struct fhip_ctx *fa_set_handle(FlakeAmdSet *g) { return g ? g->hip : NULL; }
int fa_set_max_batch(const FlakeAmdSet *g) { return g ? g->max_batch : 0; }

long long fa_set_encode_from(FlakeAmdSet *g, fa_set_source *src, int nblocks, int block_size, const int *stream_of_block,
                             unsigned char *out, size_t out_size, int *frame_sizes)
{
    if (!g || !src) return -1;
    if (g->host_md5) SET_FAIL("flake_amd_set_encode: a set that hashes on the host needs its samples there");
    src->cur = 0;
    /* (the samples pointer is the batch's token: it is compared, never followed) */
    return set_encode(g, src, (const void *)src, 4, nblocks, block_size, stream_of_block, out, out_size, frame_sizes);
}

long long fa_set_encode_short_from(FlakeAmdSet *g, fa_set_source *src, int nblocks, const int *block_sizes,
                                   const int *stream_of_block, unsigned char *out, size_t out_size, int *frame_sizes)
{
    if (!g || !src) return -1;
    g->err[0] = 0;
    g->vfail = 0;
    if (g->broken) SET_FAIL("flake_amd_set_encode_ragged: an earlier device error left the set unusable");
    if (g->host_md5) SET_FAIL("flake_amd_set_encode_ragged: a set that hashes on the host needs its samples there");
    if (nblocks < 0 || (nblocks > 0 && (!block_sizes || !stream_of_block || !out)))
        SET_FAIL("flake_amd_set_encode_ragged: null argument or negative block count");
    if (nblocks == 0) return 0;
    /* flake_amd_set_encode_ragged's checks, for a call whose blocks are all short */
    int *per = g->scratch;
    memset(per, 0, sizeof(int) * (size_t)g->nstreams);
    for (int b = 0; b < nblocks; b++) {
        const int s = stream_of_block[b], n = block_sizes[b];
        if (n < 1 || n >= g->hp.block_size) SET_FAIL("flake_amd_set_encode_ragged: block_sizes[%d] = %d is not a short block", b, n);
        if (s < 0 || s >= g->nstreams) SET_FAIL("flake_amd_set_encode_ragged: stream_of_block[%d] = %d is outside the set's %d streams", b, s, g->nstreams);
        if (g->ended[s] || per[s])
            SET_FAIL("flake_amd_set_encode_ragged: block %d belongs to stream %d, which a short block has ended", b, s);
        per[s] = 1;
    }
    src->cur = 0;
    const long long r = set_encode_short(g, src, (const void *)src, 4, nblocks, block_sizes, stream_of_block, out, out_size,
                                         frame_sizes);
    if (r == -2) SET_FAIL("flake_amd_set_encode_ragged: the ragged packed path does not cover this set (block size above 16384)");
    return r;
}

/* ---- encode rows: a planar batch on the device (host/rows_plan.h, K12) ---- */

/* The rows become two calls' worth of blocks -- every row's whole blocks, then every row's short block -- and each part
 * runs through the set's own path with its samples named by row pieces (fa_set_source), which set_bring() hands to
 * fhip_frames_packed_from_rows chunk by chunk.  Both parts' argument rules are held here first, against the streams as
 * they are: the whole blocks change nothing the short blocks' rules read (they end no stream). */
FLAKE_AMD_API long long flake_amd_set_encode_rows(FlakeAmdSet *g, const void *rows_dev, int format, int nrows, long long row_len,
                                                  const int *stream_of_row, const long long *len_of_row,
                                                  unsigned char *out, size_t out_size,
                                                  long long *row_whole_bytes, long long *row_tail_bytes)
{
    if (!g) return -1;
    g->err[0] = 0;
    g->vfail = 0;
    if (g->broken) SET_FAIL("flake_amd_set_encode_rows: an earlier device error left the set unusable");
    if (g->host_md5) SET_FAIL("flake_amd_set_encode_rows: a set that hashes on the host (FLAKE_AMD_SET_MD5_HOST) needs its samples there");
    if (nrows < 0 || (nrows > 0 && (!rows_dev || !stream_of_row || !len_of_row || !out || !row_whole_bytes || !row_tail_bytes)))
        SET_FAIL("flake_amd_set_encode_rows: null argument or negative row count");
    if (format != FHIP_ROWS_I32 && format != FHIP_ROWS_I16 && format != FHIP_ROWS_F32)
        SET_FAIL("flake_amd_set_encode_rows: format must be FLAKE_AMD_ROWS_I32, _I16 or _F32");
    if (format == FHIP_ROWS_I16 && g->hp.bits_per_sample > 16)
        SET_FAIL("flake_amd_set_encode_rows: int16 rows need bits_per_sample <= 16");
    if (nrows == 0) return 0;
    if (row_len < 1 || row_len > INT32_MAX) SET_FAIL("flake_amd_set_encode_rows: row_len out of range");
    const int B = g->hp.block_size;
    int *per = g->scratch;                /* 1: the stream has a short block in this call */
    memset(per, 0, sizeof(int) * (size_t)g->nstreams);
    for (int r = 0; r < nrows; r++) {
        const int s = stream_of_row[r];
        const long long len = len_of_row[r];
        if (len < 0 || len > row_len) SET_FAIL("flake_amd_set_encode_rows: len_of_row[%d] = %lld is outside the row's %lld columns", r, len, row_len);
        if (s < 0 || s >= g->nstreams) SET_FAIL("flake_amd_set_encode_rows: stream_of_row[%d] = %d is outside the set's %d streams", r, s, g->nstreams);
        if (len == 0) continue;
        if (g->ended[s]) SET_FAIL("flake_amd_set_encode_rows: row %d belongs to stream %d, which a short block has ended", r, s);
        if (len % B) {
            if (per[s]) SET_FAIL("flake_amd_set_encode_rows: row %d gives stream %d a second short block in one call", r, s);
            per[s] = 1;
        }
    }
    fa_rows_counts n;
    if (fa_rows_count(nrows, len_of_row, B, &n) != 0) SET_FAIL("flake_amd_set_encode_rows: too many blocks for one call");
    if (n.nshort > 0 && B > 16384)
        SET_FAIL("flake_amd_set_encode_rows: the ragged packed path does not cover this set (block size above 16384): "
                 "rows must be multiples of the block size");
    for (int r = 0; r < nrows; r++) row_whole_bytes[r] = row_tail_bytes[r] = 0;
    if (n.nwhole + n.nshort == 0) return 0;
    /* one block of int32 tables, one of pieces */
    const size_t ni = (size_t)n.nwhole * 2 + (size_t)n.nshort * 4 + (size_t)nrows + 1;
    const size_t npc = ((size_t)n.nwhole_pieces + (size_t)n.nshort) * 2;
    int32_t *tab = (int32_t *)malloc(ni * sizeof(int32_t));
    fhip_row_piece *pc = (fhip_row_piece *)malloc((npc ? npc : 1) * sizeof(fhip_row_piece));
    if (!tab || !pc) { free(tab); free(pc); SET_FAIL("flake_amd_set_encode_rows: out of host memory"); }
    int32_t *whole_stream = tab, *whole_fs = whole_stream + n.nwhole, *short_size = whole_fs + n.nwhole;
    int32_t *short_stream = short_size + n.nshort, *short_row = short_stream + n.nshort, *short_fs = short_row + n.nshort;
    int32_t *first = short_fs + n.nshort;
    fhip_row_piece *whole_pieces = pc, *short_pieces = pc + n.nwhole_pieces;
    fhip_row_piece *work = short_pieces + n.nshort;              /* room for the larger table's slice */
    fa_rows_plan(nrows, len_of_row, stream_of_row, B, whole_stream, whole_pieces, short_size, short_stream, short_pieces,
                 first, short_row);
    const fhip_rows_in rows = {rows_dev, nrows, format, row_len};
    long long total = 0;
    if (n.nwhole > 0) {
        fa_set_source src;
        memset(&src, 0, sizeof src);
        src.npieces = n.nwhole_pieces; src.rows = &rows; src.row_pieces = whole_pieces; src.row_work = work;
        const long long w = fa_set_encode_from(g, &src, n.nwhole, B, (const int *)whole_stream, out, out_size, (int *)whole_fs);
        if (w < 0) { free(tab); free(pc); return -1; }
        total = w;
        for (int r = 0; r < nrows; r++)
            for (int b = first[r]; b < first[r + 1]; b++) row_whole_bytes[r] += whole_fs[b];
    }
    if (n.nshort > 0) {
        fa_set_source src;
        memset(&src, 0, sizeof src);
        src.npieces = n.nshort; src.rows = &rows; src.row_pieces = short_pieces; src.row_work = work;
        const long long w = fa_set_encode_short_from(g, &src, n.nshort, (const int *)short_size, (const int *)short_stream,
                                                     out + total, out_size - (size_t)total, (int *)short_fs);
        if (w < 0) {
            /* the whole blocks are part of their streams already: what the caller holds no longer matches the set */
            if (n.nwhole > 0) g->broken = 1;
            free(tab); free(pc);
            return -1;
        }
        total += w;
        for (int i = 0; i < n.nshort; i++) row_tail_bytes[short_row[i]] = short_fs[i];
    }
    free(tab); free(pc);
    return total;
}

/* ---- seek points (host/seekpoints.h); not in the drop-in libflake.so ---- */
#ifndef FLAKE_AMD_EXPORT_FLAKE_NAMES
FLAKE_AMD_API int flake_amd_set_seekpoints(FlakeAmdSet *g, unsigned long long spacing)
{
    if (!g) return -1;
    for (int s = 0; s < g->nstreams; s++) if (g->samples[s] || g->ended[s]) return -1;      /* a block has been committed */
    if (!g->seek && spacing) {
        g->seek = (fa_seekrec *)calloc((size_t)g->nstreams, sizeof(fa_seekrec));
        if (!g->seek) return -1;
    }
    if (g->seek) for (int s = 0; s < g->nstreams; s++) fa_seekrec_init(&g->seek[s], spacing);
    g->seek_fmt.channels = g->hp.channels; g->seek_fmt.bps = g->hp.bits_per_sample;
    g->seek_fmt.sample_rate = g->hp.sample_rate; g->seek_fmt.max_block_size = 0;
    return 0;
}

FLAKE_AMD_API long long flake_amd_set_get_seekpoints(const FlakeAmdSet *g, int stream, FlakeAmdSeekPoint *p, int cap)
{
    if (!g || stream < 0 || stream >= g->nstreams || cap < 0 || (cap > 0 && !p)) return -1;
    return g->seek ? fa_seekrec_get(&g->seek[stream], p, cap) : 0;
}
#endif

FLAKE_AMD_API int flake_amd_set_get_streaminfo(FlakeAmdSet *g, int stream, FlakeAmdStreaminfo *si)
{
    if (!g || !si) return -1;
    g->err[0] = 0;
    if (stream < 0 || stream >= g->nstreams) SET_FAIL("flake_amd_set_get_streaminfo: no stream %d in a set of %d", stream, g->nstreams);
    if (!g->digests_valid) {
        /* one finalisation and one read-back for ALL streams: a caller walking the set pays one synchronisation */
        const int rc = fhip_md5_final(g->hip, g->dev_md5, g->nstreams, g->digests);
        if (rc != FHIP_OK) SET_FAIL("fhip_md5_final: %s (%s)", fhip_strerror(rc), fhip_last_error(g->hip));
        g->digests_valid = 1;
    }
    si->min_block_size = g->vbs ? 16u : (unsigned)g->hp.block_size;   /* as flake_amd_get_streaminfo reports it */
    si->max_block_size = (unsigned)g->hp.block_size;
    si->min_frame_size = 0;                                       /* as flake_amd_get_streaminfo leaves it */
    si->max_frame_size = (unsigned)g->max_frame[stream];
    si->sample_rate = (unsigned)g->hp.sample_rate;
    si->channels = (unsigned)g->hp.channels;
    si->bits_per_sample = (unsigned)g->hp.bits_per_sample;
    si->samples = (unsigned)g->samples[stream];
    memcpy(si->md5sum, g->digests + 16 * (size_t)stream, 16);     /* zeros under FLAKE_AMD_SET_MD5_OFF */
    return 0;
}
