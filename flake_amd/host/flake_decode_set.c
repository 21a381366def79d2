/*
 * flake_decode_set.c -- a decode set: the frames of many streams of one format decoded in shared device batches
 * (fhip_decode_frames_segments: K7's segment mode), each stream's MD5 carried on the device (K6, k_md5_ranges, fed by
 * the ranges K7 leaves there).  The counterpart of flake_set.c on the decoding side.
 *
 * The planner (decode_set_plan.h) cuts a call into batches and writes the tables; this file owns the handle, the
 * streams' states and what a batch's results mean for them: a failing frame fails its stream, for good, and no other.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"
#include "flakehip.h"
#include "host_internal.h"
#include "decode_set_plan.h"
#include "decode_window_plan.h"
#include "decode_window_place.h"
#include "held_plan.h"
#include "span_rows_plan.h"

typedef struct {
    long long frames_done;        /* frames committed so far */
    long long fail_frame;         /* failed: the frame, counted from the stream's first, and its status */
    int fail_status;
    fa_md5 md5;                   /* FLAKE_AMD_SET_MD5_HOST */
} ds_stream;

struct FlakeAmdDecodeSet {
    fhip_ctx *hip;
    FlakeAmdStreaminfo si;
    int nstreams, max_batch;
    unsigned flags;
    void *tables;                 /* one block: every table below that nstreams or max_batch sizes (ds_carve) */
    fa_ds_stream *st;             /* what the planner reads */
    ds_stream *sx;                /* the rest */
    fhip_md5_state *states;       /* device: one per stream (neither _HOST nor _OFF) */
    unsigned char *digests;       /* [nstreams][16], valid while have_digests */
    int have_digests;
    long long device_batches;
    fa_ds_batch b;                /* the planner's tables and the device's answers, max_batch entries each */
    int64_t *seg_start, *seg_samples;
    int32_t *seg_failed;
    unsigned char *seg_ok;        /* what the set made of each segment of the batch (the keep form's consumer reads it) */
    int max_block;                /* the handle's largest block */
    fhip_verify_rec *recs;
    long long *run_off;           /* the last call's run offsets in pcm */
    int run_off_cap, run_off_n;
    /* flake_amd_decode_set_windows: the planner's tables (max_batch entries each), the selections and the runs' tables
     * (one per window: one block, wtables, grown on demand), the offsets of the call's frames and the staged bytes of a
     * batch */
    fa_dw_batch wb;
    void *wtables;
    int wcap;
    fa_dw_sel *wsel;
    const unsigned char **wdata;
    const int **wsizes;
    const size_t **woff;
    long long *wat;
    size_t *foff;
    size_t foff_cap;
    unsigned char *wstage;
    size_t wstage_cap;
    int32_t *wfb;
    int32_t *wstat;               /* each segment's failing frame's status, and where its samples belong (decode_window_place.h) */
    long long *wtarget;
    int32_t *wrow;                /* flake_amd_decode_set_windows_rows: each segment's row and first column */
    int64_t *wcol;
    int32_t *wnrows;              /* flake_amd_decode_set_span_rows: each segment's span's rows [max_batch], every span's
                                   * first row [per span, and the end] and what it has delivered [per span] */
    int32_t *wspanrow;
    long long *wspansmp;
    /* held streams (flake_amd_decode_set_hold ...): the store on the device, and the host's table of what it holds --
     * every stream's entry, every frame's size and head, every frame's offset in the store (and each stream's end) */
    unsigned char *hstore;
    size_t hcap, hused;
    fa_held_stream *hs;
    size_t hs_cap;
    int hn;
    int32_t *hsize;
    fa_held_head *hhead;
    size_t *hoff;
    size_t hsize_cap, hhead_cap, hoff_cap;
    long long hframes, hoffs;     /* entries in use */
    long long hup_add, hup_win;   /* bytes uploaded by hold_add and by held window calls */
    int64_t *wsrc;                /* a held batch's frames' offsets in the store [max_batch] */
    long long *wfirst;            /* a held call's windows' first records [per window] */
    char err[384];
};

typedef char ds_header_status_agrees[(int)FA_WP_HEADER == (int)FHIP_VERIFY_HEADER ? 1 : -1];
typedef char ds_held_head_agrees[sizeof(fa_held_head) == sizeof(fhip_frame_head) && sizeof(fa_held_head) == 16 ? 1 : -1];

static char g_open_err[256];

static int ds_device_md5(const FlakeAmdDecodeSet *g) { return !(g->flags & (FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF)); }

/* One table of a block: count elements of elem bytes at *at, which moves on to the next 8-byte boundary behind them.
 * Without a block (base NULL) only the sizes add up. */
static void *ds_slot(unsigned char *base, size_t *at, size_t count, size_t elem)
{
    void *p = base ? base + *at : NULL;
    *at += (count * elem + 7) & ~(size_t)7;
    return p;
}
#define DS_SLOT(p, count) ((p) = ds_slot(base, &at, (count), sizeof *(p)))

/* The tables of fixed size, [nstreams] and [max_batch] ones, in one block at base.  Returns the block's size. */
static size_t ds_carve(FlakeAmdDecodeSet *g, unsigned char *base)
{
    const size_t mb = (size_t)g->max_batch, ns = (size_t)g->nstreams;
    fa_ds_batch *b = &g->b;
    fa_dw_batch *wb = &g->wb;
    size_t at = 0;
    DS_SLOT(g->st, ns); DS_SLOT(g->sx, ns);
    g->digests = (unsigned char *)ds_slot(base, &at, ns, 16);
    DS_SLOT(b->seg_first, mb + 1); DS_SLOT(b->seg_number, mb); DS_SLOT(b->seg_variable, mb); DS_SLOT(b->seg_stream, mb);
    DS_SLOT(b->seg_run, mb); DS_SLOT(b->seg_frame0, mb); DS_SLOT(b->seg_prev, mb);
    DS_SLOT(b->md5_first, ns + 1); DS_SLOT(b->md5_range, mb); DS_SLOT(b->last_seg, ns); DS_SLOT(b->planned, ns);
    DS_SLOT(g->seg_start, mb); DS_SLOT(g->seg_samples, mb); DS_SLOT(g->seg_failed, mb); DS_SLOT(g->recs, mb);
    DS_SLOT(g->seg_ok, mb);
    DS_SLOT(wb->seg_first, mb + 1); DS_SLOT(wb->seg_number, mb); DS_SLOT(wb->seg_variable, mb); DS_SLOT(wb->seg_skip, mb);
    DS_SLOT(wb->seg_take, mb); DS_SLOT(wb->seg_win, mb); DS_SLOT(wb->seg_frame0, mb); DS_SLOT(wb->seg_last, mb);
    DS_SLOT(g->wfb, mb); DS_SLOT(g->wstat, mb); DS_SLOT(g->wtarget, mb); DS_SLOT(g->wrow, mb); DS_SLOT(g->wcol, mb);
    DS_SLOT(g->wsrc, mb); DS_SLOT(g->wnrows, mb);
    return at;
}

/* The tables with an entry per window, n of them, likewise. */
static size_t ds_carve_windows(FlakeAmdDecodeSet *g, unsigned char *base, size_t n)
{
    size_t at = 0;
    DS_SLOT(g->wsel, n); DS_SLOT(g->wdata, n); DS_SLOT(g->wsizes, n); DS_SLOT(g->woff, n); DS_SLOT(g->wat, n);
    DS_SLOT(g->wfirst, n); DS_SLOT(g->wspanrow, n + 1); DS_SLOT(g->wspansmp, n);
    return at;
}

FLAKE_AMD_API FlakeAmdDecodeSet *flake_amd_decode_set_open(const FlakeAmdStreaminfo *like, int nstreams, unsigned flags)
{
    g_open_err[0] = 0;
    if (!like || like->channels < 1 || like->channels > 8 || like->bits_per_sample < 4 || like->bits_per_sample > 32 ||
        like->sample_rate < 1 || like->sample_rate > 655350u || like->max_block_size > 65535u) {
        snprintf(g_open_err, sizeof g_open_err, "STREAMINFO is out of range");
        return NULL;
    }
    if (nstreams < 1 || nstreams > (1 << 20)) {
        snprintf(g_open_err, sizeof g_open_err, "nstreams out of range");
        return NULL;
    }
    if ((flags & ~(FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF)) ||
        (flags & (FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF)) == (FLAKE_AMD_SET_MD5_HOST | FLAKE_AMD_SET_MD5_OFF)) {
        snprintf(g_open_err, sizeof g_open_err, "unknown or contradictory flags");
        return NULL;
    }
    FlakeAmdDecodeSet *g = (FlakeAmdDecodeSet *)calloc(1, sizeof *g);
    if (!g) return NULL;
    g->si = *like;
    g->nstreams = nstreams;
    g->flags = flags;
    const char *eb = getenv("FLAKE_AMD_BATCH"), *ed = getenv("FLAKE_AMD_DEVICE");
    g->max_batch = eb ? atoi(eb) : 1024;
    if (g->max_batch < 1) g->max_batch = 1;
    /* the handle, as flake_amd_decode_open makes it */
    int bs = like->max_block_size ? (int)like->max_block_size : 65535;
    if (bs < 16) bs = 16;
    if ((long long)g->max_batch * bs > (4ll << 20)) g->max_batch = (int)((4ll << 20) / bs);
    if (g->max_batch < 1) g->max_batch = 1;
    fhip_params p;
    memset(&p, 0, sizeof p);
    p.channels = (int)like->channels; p.sample_rate = (int)like->sample_rate; p.bits_per_sample = (int)like->bits_per_sample;
    g->max_block = bs;
    p.block_size = bs; p.order_method = 1; p.stereo_method = 1; p.prediction_type = 2;
    p.min_prediction_order = 1; p.max_prediction_order = 8; p.min_partition_order = 0; p.max_partition_order = 5;
    p.lpc_precision = 15;
    g->tables = calloc(1, ds_carve(g, NULL));
    if (g->tables) ds_carve(g, (unsigned char *)g->tables);
    int rc = g->tables ? fhip_create(&g->hip, ed ? atoi(ed) : 0, &p, g->max_batch) : FHIP_E_NOMEM;
    if (rc == FHIP_OK && ds_device_md5(g)) {
        g->states = (fhip_md5_state *)fhip_device_alloc((size_t)nstreams * sizeof(fhip_md5_state));
        rc = g->states ? fhip_md5_init_dev(g->hip, g->states, nstreams) : FHIP_E_NOMEM;
        if (rc == FHIP_OK) rc = fhip_sync(g->hip);
    }
    if (rc != FHIP_OK) {
        snprintf(g_open_err, sizeof g_open_err, "%s", g->hip ? fhip_last_error(g->hip) : fhip_strerror(rc));
        flake_amd_decode_set_close(g);
        return NULL;
    }
    for (int s = 0; s < nstreams; s++) { fa_md5_init(&g->sx[s].md5); g->sx[s].fail_frame = -1; }
    return g;
}

static void ds_fail_stream(FlakeAmdDecodeSet *g, int s, long long frame, int status)
{
    if (g->st[s].failed) return;
    g->st[s].failed = 1;
    g->sx[s].fail_frame = frame;
    g->sx[s].fail_status = status;
}

/* What both sinks refuse of the samples' width; bad_argument: the call's own null and range checks, first in line. */
static int ds_refuse_samples(FlakeAmdDecodeSet *g, int bad_argument, int sample_bytes)
{
    if (bad_argument || (sample_bytes != 2 && sample_bytes != 4)) {
        snprintf(g->err, sizeof g->err, "bad argument");
        return -1;
    }
    if (sample_bytes == 2 && g->si.bits_per_sample > 16) {
        snprintf(g->err, sizeof g->err, "2-byte samples need bits_per_sample <= 16");
        return -1;
    }
    return 0;
}

/* The rest of what flake_amd_decode_set_frames refuses, and what it needs before it changes the set. */
static int ds_frames_begin(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run, const int *frames_of_run,
                           const int *frame_sizes, size_t bytes, int sample_bytes)
{
    long long total_frames = 0;
    const int chk = fa_ds_check(g->nstreams, g->st, nruns, stream_of_run, frames_of_run, frame_sizes, bytes, &total_frames);
    if (chk != FA_DS_OK) {
        snprintf(g->err, sizeof g->err, "%s",
                 chk == FA_DS_BAD_STREAM ? "a run names a stream outside the set" :
                 chk == FA_DS_BAD_SIZE ? "the frame sizes run past the stream" :
                 chk == FA_DS_FAILED_STREAM ? "a run names a stream that has failed" : "bad argument");
        return -1;
    }
    if (nruns > g->run_off_cap) {
        long long *n = (long long *)realloc(g->run_off, sizeof(long long) * (size_t)nruns);
        if (!n) { snprintf(g->err, sizeof g->err, "out of memory"); return -1; }
        g->run_off = n;
        g->run_off_cap = nruns;
    }
    if (fhip_set_pcm_format(g->hip, sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32) != FHIP_OK) {
        snprintf(g->err, sizeof g->err, "%s", fhip_last_error(g->hip));
        return -1;
    }
    return 0;
}

/* A stream seen for the first time tells its blocking strategy and first number in its first frame. */
static void ds_first_frames(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run, const int *frames_of_run,
                            const unsigned char *stream, const int *frame_sizes)
{
    size_t at = 0;
    long long f = 0;
    for (int r = 0; r < nruns; r++) {
        const int s = stream_of_run[r];
        if (frames_of_run[r] > 0 && !g->st[s].started && !g->st[s].failed) {
            flac_header h;
            if (fa_parse_header(&g->si, stream + at, (size_t)frame_sizes[f], &h)) {
                /* not a header this parser takes: the device decides what is wrong with it (its status is the
                 * stream's, as for any later frame); it is shown the strategy bit the frame carries */
                g->st[s].variable = frame_sizes[f] >= 2 ? (stream[at + 1] & 1) : 0;
            } else {
                g->st[s].started = 1;
                g->st[s].variable = h.vbs;
                g->st[s].next_number = (long long)h.number;
            }
        }
        for (int k = 0; k < frames_of_run[r]; k++) at += (size_t)frame_sizes[f++];
    }
}

/* The batch's segments in order, once the device has answered: a good one commits its stream, a bad one fails it.
 * base: where the batch's samples begin in pcm.  Returns how far the good segments reach from there. */
static size_t ds_judge_batch(FlakeAmdDecodeSet *g, const unsigned char *stream, const int *frame_sizes, const void *pcm,
                             int sample_bytes, size_t base, long long *run_samples)
{
    const fa_ds_batch *b = &g->b;
    const size_t nch = g->si.channels;
    const int bps = (int)g->si.bits_per_sample;
    size_t extent = 0;
    size_t hdr_at = b->byte0;
    memset(g->seg_ok, 0, (size_t)b->nsegs);
    for (int k = 0; k < b->nsegs; k++) {
        const int s = b->seg_stream[k], r = b->seg_run[k];
        const int nf = b->seg_first[k + 1] - b->seg_first[k];
        fa_ds_stream *t = &g->st[s];
        const size_t seg_bytes_at = hdr_at;
        for (int f = b->seg_first[k]; f < b->seg_first[k + 1]; f++) hdr_at += (size_t)frame_sizes[b->frame0 + f];
        if (!t->failed && g->seg_failed[k] >= 0) {
            const int bad = g->seg_failed[k];
            ds_fail_stream(g, s, g->sx[s].frames_done + (bad - b->seg_first[k]), (int)g->recs[bad].status);
        }
        if (!t->failed && b->seg_number[k] < 0 && b->seg_prev[k] >= 0) {
            /* a variable-block-size stream's later segment of the batch: numbered on from the earlier one */
            flac_header h;
            if (fa_parse_header(&g->si, stream + seg_bytes_at, (size_t)frame_sizes[b->frame0 + b->seg_first[k]], &h) ||
                (long long)h.number != t->next_number)
                ds_fail_stream(g, s, g->sx[s].frames_done, FHIP_VERIFY_NUMBER);
        }
        if (!t->failed && !t->started)       /* the device took a first frame that the CPU parser did not */
            ds_fail_stream(g, s, g->sx[s].frames_done, FHIP_VERIFY_HEADER);
        if (!t->failed && !t->variable) {
            /* fixed blocks: the size rule from segment to segment (fa_ds_fixed_sizes), on the first and last header */
            flac_header h0, h1;
            const size_t last_bytes = (size_t)frame_sizes[b->frame0 + b->seg_first[k + 1] - 1];
            if (fa_parse_header(&g->si, stream + seg_bytes_at, (size_t)frame_sizes[b->frame0 + b->seg_first[k]], &h0) ||
                fa_parse_header(&g->si, stream + hdr_at - last_bytes, last_bytes, &h1) ||
                fa_ds_fixed_sizes(t, nf, h0.n, h1.n))
                ds_fail_stream(g, s, g->sx[s].frames_done, FHIP_VERIFY_NUMBER);
        }
        if (t->failed) {
            run_samples[r] = -1;
            continue;
        }
        g->seg_ok[k] = 1;
        const size_t at = base + (size_t)g->seg_start[k], n = (size_t)g->seg_samples[k];
        if (b->seg_frame0[k] == 0) g->run_off[r] = (long long)at;
        if (g->flags & FLAKE_AMD_SET_MD5_HOST) {
            if (sample_bytes == 2) fa_md5_pcm16(&g->sx[s].md5, (const int16_t *)pcm + at * nch, n * nch, bps);
            else fa_md5_pcm(&g->sx[s].md5, (const int32_t *)pcm + at * nch, n * nch, bps);
        }
        t->next_number += t->variable ? (long long)n : (long long)nf;
        g->sx[s].frames_done += nf;
        run_samples[r] += (long long)n;
        if (at + n - base > extent) extent = at + n - base;
    }
    return extent;
}

/* keep_fn: the keep-on-device destination (fa_decode_set_frames_keep) -- pcm is device memory that every batch decodes
 * to from its start, and each batch is handed to keep_fn once its segments are judged. */
static long long ds_frames(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run, const int *frames_of_run,
                           const unsigned char *stream, size_t bytes, const int *frame_sizes, void *pcm, int sample_bytes,
                           size_t pcm_cap_samples, long long *run_samples, fa_ds_batch_fn keep_fn, void *keep_user)
{
    if (!g) return -1;
    g->err[0] = 0;
    if (ds_refuse_samples(g, (!stream && bytes) || (!pcm && pcm_cap_samples) || (nruns > 0 && !run_samples), sample_bytes) ||
        ds_frames_begin(g, nruns, stream_of_run, frames_of_run, frame_sizes, bytes, sample_bytes))
        return -1;
    /* from here on the call changes the set */
    g->have_digests = 0;
    g->run_off_n = nruns;
    for (int r = 0; r < nruns; r++) { run_samples[r] = 0; g->run_off[r] = -1; }
    ds_first_frames(g, nruns, stream_of_run, frames_of_run, stream, frame_sizes);
    const size_t nch = g->si.channels;
    fa_ds_cursor cur;
    memset(&cur, 0, sizeof cur);
    fa_ds_batch *b = &g->b;
    size_t base = 0;                                  /* where the batch's samples begin in pcm */
    long long total = 0;
    while (fa_ds_plan(&cur, nruns, stream_of_run, frames_of_run, frame_sizes, g->nstreams, g->st, g->max_batch, b) > 0) {
        int64_t summary[4] = {0, 0, -1, 0}, nsmp = 0;
        fhip_decode_in in = {stream + b->byte0, (int64_t)b->nbytes, frame_sizes + b->frame0, b->nframes, 0, -1};
        fhip_decode_segments sg = {b->seg_first, b->nsegs, b->seg_number, b->seg_variable, g->seg_start, g->seg_samples,
                                   g->seg_failed};
        fhip_decode_out out = {(int32_t *)((char *)pcm + base * nch * (size_t)sample_bytes),
                               (int64_t)(pcm_cap_samples - base), g->recs, summary, &nsmp};
        fhip_decode_md5 md = {g->states, g->nstreams, b->seg_stream};
        const int rc = keep_fn ? fhip_decode_frames_segments_keep(g->hip, &in, &sg, &out, ds_device_md5(g) ? &md : NULL)
                               : fhip_decode_frames_segments(g->hip, &in, &sg, &out, ds_device_md5(g) ? &md : NULL);
        g->device_batches++;
        if (rc != FHIP_OK && rc != FHIP_E_VERIFY) {
            snprintf(g->err, sizeof g->err, "fhip_decode_frames_segments: %s", fhip_last_error(g->hip));
            return -1;
        }
        const size_t extent = ds_judge_batch(g, stream, frame_sizes, pcm, sample_bytes, base, run_samples);
        if (keep_fn) {
            if (keep_fn(keep_user, b->nsegs, b->seg_stream, g->seg_start, g->seg_samples, g->seg_ok) < 0) {
                if (!g->err[0]) snprintf(g->err, sizeof g->err, "the batch's consumer failed");
                return -1;
            }
            continue;                                 /* (the next batch decodes to the buffer's start again) */
        }
        base += extent;
    }
    for (int r = 0; r < nruns; r++)
        if (run_samples[r] > 0) total += run_samples[r];              /* (a stream's runs before its failing one stand) */
    return total;
}

FLAKE_AMD_API long long flake_amd_decode_set_frames(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run,
                                                    const int *frames_of_run, const unsigned char *stream, size_t bytes,
                                                    const int *frame_sizes, void *pcm, int sample_bytes,
                                                    size_t pcm_cap_samples, long long *run_samples)
{
    return ds_frames(g, nruns, stream_of_run, frames_of_run, stream, bytes, frame_sizes, pcm, sample_bytes, pcm_cap_samples,
                     run_samples, NULL, NULL);
}

long long fa_decode_set_frames_keep(FlakeAmdDecodeSet *g, int nruns, const int *stream_of_run, const int *frames_of_run,
                                    const unsigned char *stream, size_t bytes, const int *frame_sizes, int32_t *dev_pcm,
                                    size_t dev_cap_samples, long long *run_samples, fa_ds_batch_fn fn, void *user)
{
    if (!g || !fn) return -1;
    if (g->flags & FLAKE_AMD_SET_MD5_HOST) {
        snprintf(g->err, sizeof g->err, "FLAKE_AMD_SET_MD5_HOST has no samples to hash when they stay on the device");
        return -1;
    }
    return ds_frames(g, nruns, stream_of_run, frames_of_run, stream, bytes, frame_sizes, dev_pcm, 4, dev_cap_samples,
                     run_samples, fn, user);
}

size_t fa_decode_set_batch_samples(const FlakeAmdDecodeSet *g) { return (size_t)g->max_batch * (size_t)g->max_block; }
int fa_decode_set_max_batch(const FlakeAmdDecodeSet *g) { return g->max_batch; }
int fa_decode_set_max_block(const FlakeAmdDecodeSet *g) { return g->max_block; }

FLAKE_AMD_API int flake_amd_decode_set_run_offsets(const FlakeAmdDecodeSet *g, long long *offsets, int cap)
{
    if (!g || (!offsets && cap > 0)) return -1;
    for (int r = 0; r < g->run_off_n && r < cap; r++) offsets[r] = g->run_off[r];
    return g->run_off_n;
}

FLAKE_AMD_API int flake_amd_decode_set_md5(FlakeAmdDecodeSet *g, int stream, unsigned char md5[16])
{
    if (!g || !md5 || stream < 0 || stream >= g->nstreams) return -1;
    if (g->flags & FLAKE_AMD_SET_MD5_OFF) {
        snprintf(g->err, sizeof g->err, "the set was opened with FLAKE_AMD_SET_MD5_OFF: it has no digest");
        return -1;
    }
    if (g->st[stream].failed) {
        snprintf(g->err, sizeof g->err, "stream %d has failed: it has no digest", stream);
        return -1;
    }
    if (g->flags & FLAKE_AMD_SET_MD5_HOST) {
        fa_md5_final(&g->sx[stream].md5, md5);
        return 0;
    }
    if (!g->have_digests) {                           /* every stream's at once: one launch, one copy, one wait */
        if (fhip_md5_final(g->hip, g->states, g->nstreams, g->digests) != FHIP_OK) {
            snprintf(g->err, sizeof g->err, "fhip_md5_final: %s", fhip_last_error(g->hip));
            return -1;
        }
        g->have_digests = 1;
    }
    memcpy(md5, g->digests + (size_t)stream * 16, 16);
    return 0;
}

FLAKE_AMD_API int flake_amd_decode_set_failed(const FlakeAmdDecodeSet *g, int stream, long long *frame, int *status)
{
    if (!g || stream < 0 || stream >= g->nstreams) return -1;
    if (!g->st[stream].failed) return 0;
    if (frame) *frame = g->sx[stream].fail_frame;
    if (status) *status = g->sx[stream].fail_status;
    return 1;
}

FLAKE_AMD_API long long flake_amd_decode_set_device_batches(const FlakeAmdDecodeSet *g)
{
    return g ? g->device_batches : -1;
}

/* ---- windows ------------------------------------------------------------------------------------------------------
 * Stateless, as flake_amd_decode_set_index is: the set lends its handle and its format.  decode_window_plan.h selects
 * the frames and cuts the batches; each batch's selected bytes are staged back to back and go through
 * fhip_decode_frames_windows, which delivers the batch's clips back to back where the call's output has got to.
 * decode_window_place.h says where each clip belongs -- a window that failed keeps the room it asked for -- and what the
 * batch left behind such a window is moved up by the difference.
 *
 * The rows sink (flake_amd_decode_set_windows_rows) is the same loop with another destination: window w is row w of a
 * device buffer, each batch goes through fhip_decode_frames_windows_rows with the segment's window as its row and what
 * the window has delivered so far as its column, and nothing is moved on the host.  The destination is zeroed on the
 * handle's stream before the first batch and a failed window's row again at the end, so that whatever no good window
 * delivered is zero.
 *
 * Span rows (flake_amd_decode_set_span_rows) are the rows sink with K13 behind K7 in K10's place: a span is a window of
 * any length, selected, cut, staged and placed as one, and what the window has delivered so far is the segment's
 * position in its span.  span_rows_plan.h has the rows: span s owns rows span_first_row[s] .. span_first_row[s + 1], all
 * the call's rows are zeroed before the first batch and a failed span's again at the end. */
typedef struct {
    void *dev_rows;
    int format;
    long long row_len;
    long long hop;                /* 0: window rows.  Otherwise span rows, and the rest is theirs: */
    long long rows_cap;
    int *span_first_row;          /* [nwin + 1] */
    long long *row_samples;       /* [rows_cap] */
} ds_rows_sink;

typedef struct {                  /* a call's arguments */
    int nwin;
    const int *frames_of_win;
    const unsigned char *stream;
    size_t bytes;
    const int *frame_sizes;
    const unsigned *fixed_block_size;
    const unsigned long long *first_sample;
    const long long *count;
    void *pcm;
    int sample_bytes;
    size_t pcm_cap_samples;
    const ds_rows_sink *rows;     /* (then pcm is null, sample_bytes 4, and the room is what the windows ask for) */
    long long *win_samples;
    int *win_status;
    const int *held_of_win;       /* held streams: window w is asked of this one's whole run, and frames_of_win, stream,
                                   * bytes, frame_sizes and fixed_block_size are null: the set's table has them */
} ds_win_call;

static int ds_grow(void **p, size_t *cap, size_t want, size_t elem)
{
    if (want <= *cap) return 0;
    void *n = realloc(*p, want * elem);
    if (!n) return -1;
    *p = n;
    *cap = want;
    return 0;
}

static long long ds_nomem(FlakeAmdDecodeSet *g)
{
    snprintf(g->err, sizeof g->err, "out of memory");
    return -1;
}

/* What a windows call refuses of its arguments.  Leaves the call's frames in *nf and the samples it asks for in *asked. */
static int ds_windows_check(FlakeAmdDecodeSet *g, const ds_win_call *q, long long *nf, long long *asked)
{
    const ds_rows_sink *rows = q->rows;
    const int nwin = q->nwin;
    if (rows) {
        if (rows->row_len < 1 || (!rows->dev_rows && nwin > 0) || rows->hop < 0 || rows->hop > FA_SR_MAX_HOP ||
            (rows->hop && (rows->rows_cap < 0 || !rows->span_first_row || (!rows->row_samples && rows->rows_cap))) ||
            (rows->format != FHIP_ROWS_I32 && rows->format != FHIP_ROWS_I16 && rows->format != FHIP_ROWS_F32)) {
            snprintf(g->err, sizeof g->err, "bad argument");
            return -1;
        }
        if (rows->format == FHIP_ROWS_I16 && g->si.bits_per_sample > 16) {
            snprintf(g->err, sizeof g->err, "int16 rows need bits_per_sample <= 16");
            return -1;
        }
    }
    const int held = q->held_of_win != NULL;
    if (ds_refuse_samples(g, nwin < 0 || (nwin > 0 && ((!held && (!q->frames_of_win || !q->fixed_block_size)) ||
                                                       !q->first_sample || !q->count || (!q->win_samples && !(rows && rows->hop)) ||
                                                       !q->win_status)) ||
                             (!q->stream && q->bytes) || (!q->pcm && q->pcm_cap_samples), q->sample_bytes))
        return -1;
    const long long room = rows ? 0x7FFFFFFFFFFFFFFFll : (long long)q->pcm_cap_samples;
    *nf = *asked = 0;
    for (int w = 0; w < nwin; w++) {
        if (held && (q->held_of_win[w] < 0 || q->held_of_win[w] >= g->hn)) {
            snprintf(g->err, sizeof g->err, "a window names a held stream the set does not have");
            return -1;
        }
        const int frames = held ? g->hs[q->held_of_win[w]].frames : q->frames_of_win[w];
        if (frames < 0 || q->count[w] < 0 || q->count[w] > room - *asked) {
            snprintf(g->err, sizeof g->err, "%s", frames < 0 || q->count[w] < 0 ? "negative count"
                                                  : "pcm_cap_samples is below the samples the windows ask for");
            return -1;
        }
        if (rows && !rows->hop && q->count[w] > rows->row_len) {
            snprintf(g->err, sizeof g->err, "a window asks for more than row_len samples");
            return -1;
        }
        *asked += q->count[w];
        *nf += held ? 0 : frames;                     /* (a held call brings no frame sizes: nothing to lay out) */
    }
    if (*nf && !q->frame_sizes) { snprintf(g->err, sizeof g->err, "bad argument"); return -1; }
    return 0;
}

/* Room for nf frames' offsets and nwin windows' tables: the latter grow together, in one block, or not at all. */
static int ds_windows_room(FlakeAmdDecodeSet *g, int nwin, long long nf)
{
    if (ds_grow((void **)&g->foff, &g->foff_cap, (size_t)nf + 1, sizeof(size_t))) return -1;
    if (nwin < g->wcap) return 0;
    void *n = malloc(ds_carve_windows(g, NULL, (size_t)nwin + 1));
    if (!n) {
        ds_carve_windows(g, (unsigned char *)g->wtables, (size_t)g->wcap);      /* (as they were) */
        return -1;
    }
    free(g->wtables);
    g->wtables = n;
    g->wcap = nwin + 1;
    ds_carve_windows(g, (unsigned char *)n, (size_t)g->wcap);
    return 0;
}

/* The frames' offsets, the handle's sample format and every window's selection. */
static int ds_windows_select(FlakeAmdDecodeSet *g, const ds_win_call *q, long long nf, const flac_format *fmt)
{
    size_t at = 0;
    g->foff[0] = 0;
    for (long long f = 0; f < nf; f++) {
        if (q->frame_sizes[f] < 1 || (size_t)q->frame_sizes[f] > q->bytes - at) {
            snprintf(g->err, sizeof g->err, "the frame sizes run past the stream");
            return -1;
        }
        at += (size_t)q->frame_sizes[f];
        g->foff[f + 1] = at;
    }
    if (fhip_set_pcm_format(g->hip, q->sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32) != FHIP_OK) {
        snprintf(g->err, sizeof g->err, "%s", fhip_last_error(g->hip));
        return -1;
    }
    long long f = 0;
    for (int w = 0; w < q->nwin; w++) {
        g->wdata[w] = q->stream;                      /* (the offsets count from the call's first byte) */
        g->wsizes[w] = q->frame_sizes + f;
        g->woff[w] = g->foff + f;
        fa_dw_select(fmt, q->stream, g->wsizes[w], g->woff[w], q->frames_of_win[w], q->fixed_block_size[w],
                     q->first_sample[w], q->count[w], &g->wsel[w]);
        f += q->frames_of_win[w];
    }
    return 0;
}

/* The same for a held call: every window's run is its stream's entry of the set's table. */
static int ds_held_select(FlakeAmdDecodeSet *g, const ds_win_call *q, const fa_dw_headers *hd)
{
    if (fhip_set_pcm_format(g->hip, q->sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32) != FHIP_OK) {
        snprintf(g->err, sizeof g->err, "%s", fhip_last_error(g->hip));
        return -1;
    }
    for (int w = 0; w < q->nwin; w++) {
        const fa_held_stream *t = &g->hs[q->held_of_win[w]];
        g->wdata[w] = NULL;
        g->wsizes[w] = (const int *)g->hsize + t->frame0;
        g->woff[w] = g->hoff + t->off0;               /* (the offsets count from the store's first byte) */
        g->wfirst[w] = t->frame0;
        fa_dw_select_by(hd, w, g->woff[w], t->frames, t->fixed_block_size, q->first_sample[w], q->count[w], &g->wsel[w]);
    }
    return 0;
}

/* A held batch's frames: where each lies in the store, and its size.  Returns the bytes of the tables the device entry
 * uploads for it -- its segment tables and 12 bytes a frame, each table to the next 8-byte boundary (api.hip).  rows: 0,
 * 1 for the rows sink's two tables, 2 for span rows' four. */
static long long ds_held_stage(FlakeAmdDecodeSet *g, int rows)
{
    const fa_dw_batch *b = &g->wb;
    for (int k = 0; k < b->nsegs; k++) {
        const int w = b->seg_win[k], f0 = b->seg_frame0[k], n = b->seg_first[k + 1] - b->seg_first[k];
        for (int i = 0; i < n; i++) g->wsrc[b->seg_first[k] + i] = (int64_t)g->woff[w][f0 + i];
        memcpy(g->wfb + b->seg_first[k], g->wsizes[w] + f0, (size_t)n * sizeof(int32_t));
    }
    const long long ns = b->nsegs, nf = b->nframes;
#define DS_R8(x) (((x) + 7) & ~7ll)
    return 8 * ns * 5 + DS_R8(4 * (ns + 1)) + 2 * DS_R8(4 * ns) + (rows ? 8 * ns + DS_R8(4 * ns) : 0) +
           (rows == 2 ? DS_R8(4 * ns) + DS_R8(4 * (ns + 1)) : 0) + 8 * nf + DS_R8(4 * nf);
#undef DS_R8
}

/* The batch's bytes, back to back, and its frame sizes.  Returns the bytes; -1: out of memory. */
static long long ds_windows_stage(FlakeAmdDecodeSet *g, const unsigned char *stream)
{
    const fa_dw_batch *b = &g->wb;
    if (ds_grow((void **)&g->wstage, &g->wstage_cap, b->nbytes, 1)) return -1;
    size_t sb = 0;
    for (int k = 0; k < b->nsegs; k++) {
        const int w = b->seg_win[k], f0 = b->seg_frame0[k], n = b->seg_first[k + 1] - b->seg_first[k];
        const size_t len = g->woff[w][f0 + n] - g->woff[w][f0];
        memcpy(g->wstage + sb, stream + g->woff[w][f0], len);
        memcpy(g->wfb + b->seg_first[k], g->wsizes[w] + f0, (size_t)n * sizeof(int32_t));
        sb += len;
    }
    return (long long)sb;
}

/* A failed window's row may hold what its earlier segments delivered: zero again, run by run, then wait.  first_row
 * (span rows; null: window w is row w): window w's rows are first_row[w] .. first_row[w + 1]. */
static int ds_rows_rezero(FlakeAmdDecodeSet *g, const fhip_rows_out *ro, int nwin, const int *win_status, const int32_t *first_row)
{
    int rc = FHIP_OK;
    for (int w = 0; w < nwin && rc == FHIP_OK;) {
        int e = w;
        while (e < nwin && win_status[e]) e++;
        const int32_t r0 = first_row ? first_row[w] : w, r1 = first_row ? first_row[e] : e;
        if (r1 > r0) rc = fhip_rows_zero_dev(g->hip, ro, r0, r1 - r0);
        w = e + 1;
    }
    if (rc == FHIP_OK) rc = fhip_sync(g->hip);
    if (rc != FHIP_OK) snprintf(g->err, sizeof g->err, "flake_amd_decode_set_windows_rows: %s", fhip_last_error(g->hip));
    return rc == FHIP_OK ? 0 : -1;
}

static long long ds_windows(FlakeAmdDecodeSet *g, const ds_win_call *q, long long *frames_decoded)
{
    if (!g) return -1;
    g->err[0] = 0;
    const ds_rows_sink *rows = q->rows;
    const int nwin = q->nwin;
    long long nf = 0, asked = 0;
    if (ds_windows_check(g, q, &nf, &asked)) return -1;
    const size_t pcm_cap_samples = rows ? (size_t)asked : q->pcm_cap_samples;
    if (ds_windows_room(g, nwin, nf)) return ds_nomem(g);
    const flac_format fmt = {(int)g->si.channels, (int)g->si.bits_per_sample, (int)g->si.sample_rate,
                             g->si.max_block_size > 65535u ? 0 : (int)g->si.max_block_size};
    const int held = q->held_of_win != NULL;
    const fa_dw_bytes by = {&fmt, (const unsigned char *const *)g->wdata, (const int *const *)g->wsizes,
                            (const size_t *const *)g->woff};
    const fa_held_table tab = {g->hhead, g->wfirst};
    const fa_dw_headers hd = {held ? fa_held_get : fa_dw_bytes_get, held ? (const void *)&tab : (const void *)&by};
    if (held ? ds_held_select(g, q, &hd) : ds_windows_select(g, q, nf, &fmt)) return -1;
    const size_t unit = g->si.channels * (size_t)q->sample_bytes;
    /* span rows: every span's rows, held against the caller's room before anything is written */
    const int spans = rows && rows->hop;
    long long nrows = nwin;
    if (spans && (nrows = fa_sr_first_rows(nwin, q->count, rows->row_len, rows->hop, rows->rows_cap, g->wspanrow)) < 0) {
        snprintf(g->err, sizeof g->err, "the spans have more rows than rows_cap or than 2^31 - 1");
        return -1;
    }
    long long *const win_samples = spans ? g->wspansmp : q->win_samples;
    fa_dw_cursor cur;
    memset(&cur, 0, sizeof cur);
    fa_dw_batch *b = &g->wb;
    fa_wp_state place;
    fa_wp_begin(&place, nwin, g->wsel, q->count, g->wat, win_samples, q->win_status);
    /* from here on the rows sink writes: everything is zero before the first batch delivers */
    fhip_rows_out ro = {rows ? rows->dev_rows : NULL, (int32_t)nrows, rows ? rows->format : 0, rows ? rows->row_len : 0};
    const fhip_span_rows sp = {g->wrow, g->wnrows, g->wcol, spans ? rows->hop : 0, NULL, 0};
    if (rows && nrows > 0 && fhip_rows_zero_dev(g->hip, &ro, 0, (int32_t)nrows) != FHIP_OK) {
        snprintf(g->err, sizeof g->err, "fhip_rows_zero_dev: %s", fhip_last_error(g->hip));
        return -1;
    }
    long long decoded = 0;
    while ((!spans || nrows > 0) &&
           fa_dw_plan_by(&cur, nwin, g->wsel, &hd, (const size_t *const *)g->woff, g->max_batch, b) > 0) {
        const long long sb = held ? ds_held_stage(g, spans ? 2 : rows != NULL) : ds_windows_stage(g, q->stream);
        if (sb < 0) return ds_nomem(g);
        if (held) g->hup_win += sb;
        /* the device writes the batch's clips from base on; with rows, a window continues where its earlier segments got to */
        const long long base = fa_wp_batch(&place, b->nsegs, b->seg_win, rows ? g->wrow : NULL, rows ? g->wcol : NULL);
        if (spans) fa_sr_batch(b->nsegs, g->wspanrow, g->wrow, g->wnrows);
        int64_t summary[4] = {0, 0, -1, 0}, nsmp = 0;
        fhip_decode_in in = {g->wstage, (int64_t)sb, g->wfb, b->nframes, 0, -1};
        fhip_decode_segments sg = {b->seg_first, b->nsegs, b->seg_number, b->seg_variable, g->seg_start, g->seg_samples,
                                   g->seg_failed};
        fhip_decode_windows wn = {b->seg_skip, b->seg_take};
        fhip_decode_out out = {rows ? NULL : (int32_t *)((char *)q->pcm + (size_t)base * unit), (int64_t)pcm_cap_samples - base,
                               g->recs, summary, &nsmp};
        const int rc =
            spans ? (held ? fhip_decode_frames_windows_spans_held(g->hip, g->hstore, (int64_t)g->hused, g->wsrc, g->wfb,
                                                                  b->nframes, &sg, &wn, &sp, &ro, &out)
                          : fhip_decode_frames_windows_spans(g->hip, &in, &sg, &wn, &sp, &ro, &out)) :
            held ? (rows ? fhip_decode_frames_windows_rows_held(g->hip, g->hstore, (int64_t)g->hused, g->wsrc, g->wfb, b->nframes,
                                                                &sg, &wn, g->wrow, g->wcol, &ro, &out)
                         : fhip_decode_frames_windows_held(g->hip, g->hstore, (int64_t)g->hused, g->wsrc, g->wfb, b->nframes,
                                                           &sg, &wn, &out))
                 : (rows ? fhip_decode_frames_windows_rows(g->hip, &in, &sg, &wn, g->wrow, g->wcol, &ro, &out)
                         : fhip_decode_frames_windows(g->hip, &in, &sg, &wn, &out));
        g->device_batches++;
        decoded += b->nframes;
        if (rc != FHIP_OK && rc != FHIP_E_VERIFY) {
            snprintf(g->err, sizeof g->err, "fhip_decode_frames_windows: %s", fhip_last_error(g->hip));
            return -1;
        }
        for (int k = 0; k < b->nsegs; k++) g->wstat[k] = g->seg_failed[k] >= 0 ? (int32_t)g->recs[g->seg_failed[k]].status : 0;
        fa_wp_answers(&place, b->nsegs, b->seg_win, b->seg_last, g->seg_samples, g->seg_failed, g->wstat, g->wtarget);
        for (int k = b->nsegs - 1; k >= 0 && !rows; k--) {    /* targets never lie before the sources: from the back */
            const long long src = base + g->seg_start[k], dst = g->wtarget[k];
            if (dst >= 0 && g->seg_samples[k] > 0 && dst != src)
                memmove((char *)q->pcm + (size_t)dst * unit, (char *)q->pcm + (size_t)src * unit,
                        (size_t)g->seg_samples[k] * unit);
        }
    }
    const long long total = fa_wp_end(&place);
    if (rows && nrows > 0 && ds_rows_rezero(g, &ro, nwin, q->win_status, spans ? g->wspanrow : NULL)) return -1;
    if (frames_decoded) *frames_decoded = decoded;
    if (spans) {
        fa_sr_lengths(nwin, g->wspanrow, win_samples, rows->row_len, rows->hop, rows->row_samples);
        for (int w = 0; w <= nwin; w++) rows->span_first_row[w] = g->wspanrow[w];
        return nrows;
    }
    return total;
}

FLAKE_AMD_API long long flake_amd_decode_set_windows(FlakeAmdDecodeSet *g, int nwin, const int *frames_of_win,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count,
        void *pcm, int sample_bytes, size_t pcm_cap_samples,
        long long *win_samples, int *win_status, long long *frames_decoded)
{
    const ds_win_call q = {nwin, frames_of_win, stream, bytes, frame_sizes, fixed_block_size, first_sample, count, pcm,
                           sample_bytes, pcm_cap_samples, NULL, win_samples, win_status, NULL};
    return ds_windows(g, &q, frames_decoded);
}

FLAKE_AMD_API long long flake_amd_decode_set_windows_rows(FlakeAmdDecodeSet *g, int nwin, const int *frames_of_win,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count,
        void *dev_rows, int row_format, long long row_len,
        long long *win_samples, int *win_status, long long *frames_decoded)
{
    const ds_rows_sink sink = {dev_rows, row_format, row_len, 0, 0, NULL, NULL};
    const ds_win_call q = {nwin, frames_of_win, stream, bytes, frame_sizes, fixed_block_size, first_sample, count, NULL, 4, 0,
                           &sink, win_samples, win_status, NULL};
    return ds_windows(g, &q, frames_decoded);
}

/* ---- held streams ---------------------------------------------------------------------------------------------------
 * The store is one device allocation that streams are appended to; the host keeps, per stream, where its frames lie in
 * the set's tables, and per frame its size, its offset in the store and its header as k_frame_heads read it.  A window
 * call selects and cuts batches over that table (held_plan.h) and sends the device the frames' offsets and sizes; the
 * bytes never cross the link again. */
FLAKE_AMD_API int flake_amd_decode_set_hold(FlakeAmdDecodeSet *g, size_t capacity_bytes)
{
    if (!g) return -1;
    g->err[0] = 0;
    if (g->hstore || capacity_bytes < 1) {
        snprintf(g->err, sizeof g->err, "%s", g->hstore ? "the set holds a store already" : "bad argument");
        return -1;
    }
    g->hstore = (unsigned char *)fhip_device_alloc(capacity_bytes);
    if (!g->hstore) {
        snprintf(g->err, sizeof g->err, "no device memory for a store of %zu bytes", capacity_bytes);
        return -1;
    }
    g->hcap = capacity_bytes;
    return 0;
}

FLAKE_AMD_API long long flake_amd_decode_set_hold_add(FlakeAmdDecodeSet *g, unsigned max_block_size, const unsigned char *stream,
                                                      const size_t *range_first, int nranges, const unsigned *fixed_block_size,
                                                      int *held_ids)
{
    if (!g) return -1;
    g->err[0] = 0;
    if (!g->hstore || !range_first || nranges < 1 || !fixed_block_size || !held_ids || range_first[0] != 0 ||
        (!stream && range_first[nranges]) || g->hn > 0x7FFFFFFF - nranges) {
        snprintf(g->err, sizeof g->err, "%s", g && !g->hstore ? "the set holds no store" : "bad argument");
        return -1;
    }
    for (int r = 0; r < nranges; r++)
        if (range_first[r + 1] < range_first[r]) { snprintf(g->err, sizeof g->err, "bad argument"); return -1; }
    const size_t bytes = range_first[nranges], nr = (size_t)nranges;
    if (bytes >= ((size_t)1 << 31)) {
        snprintf(g->err, sizeof g->err, "the device indexes less than 2 GiB per call");
        return -1;
    }
    if (bytes > g->hcap - g->hused) {
        snprintf(g->err, sizeof g->err, "the store has %zu bytes left, the call brings %zu", g->hcap - g->hused, bytes);
        return -1;
    }
    /* no frame is shorter than a header, a subframe and the CRC-16: room for as many as the bytes can hold */
    size_t cap = bytes / 9 + nr + 1;
    if (cap > 0x7FFFFFFFu) cap = 0x7FFFFFFFu;
    int64_t *w = (int64_t *)malloc((2 * nr + 1) * sizeof(int64_t) + 2 * nr * sizeof(int32_t));
    if (!w || ds_grow((void **)&g->hs, &g->hs_cap, (size_t)g->hn + nr, sizeof *g->hs) ||
        ds_grow((void **)&g->hsize, &g->hsize_cap, (size_t)g->hframes + cap, sizeof *g->hsize) ||
        ds_grow((void **)&g->hhead, &g->hhead_cap, (size_t)g->hframes + cap, sizeof *g->hhead) ||
        ds_grow((void **)&g->hoff, &g->hoff_cap, (size_t)g->hoffs + cap + nr, sizeof *g->hoff)) {
        free(w);
        return ds_nomem(g);
    }
    int64_t *first = w, *cons = w + nr + 1;
    int32_t *frames = (int32_t *)(w + 2 * nr + 1), *variable = frames + nr;
    for (size_t r = 0; r <= nr; r++) first[r] = (int64_t)range_first[r];
    int32_t *sizes = g->hsize + g->hframes;
    fa_held_head *heads = g->hhead + g->hframes;
    const fhip_hold_in in = {g->hstore, (int64_t)g->hcap, (int64_t)g->hused, stream, (int64_t)bytes, first, nranges,
                             (int32_t)(max_block_size > 65535u ? 65535u : max_block_size), (int32_t)cap};
    const fhip_hold_out out = {sizes, (fhip_frame_head *)heads, frames, cons, variable};
    const int rc = fhip_hold_frames(g->hip, &in, &out);
    long long total = 0;
    for (size_t r = 0; r < nr && rc == FHIP_OK; r++) total += frames[r] > 0 ? frames[r] : 0;
    if (rc != FHIP_OK || (size_t)total > cap) {
        if (rc != FHIP_OK) snprintf(g->err, sizeof g->err, "fhip_hold_frames: %s", fhip_last_error(g->hip));
        else snprintf(g->err, sizeof g->err, "more frames than the bytes can hold");
        free(w);
        return -1;
    }
    /* from here on the call changes the set */
    long long f = 0;
    for (size_t r = 0; r < nr; r++) {
        fa_held_stream *t = &g->hs[g->hn];
        held_ids[r] = g->hn++;
        t->frame0 = g->hframes + f;
        t->off0 = g->hoffs;
        t->frames = frames[r] > 0 ? frames[r] : 0;
        t->fixed_block_size = fixed_block_size[r];
        t->samples = 0;
        size_t at = g->hused + range_first[r];
        for (int k = 0; k < t->frames; k++, f++) {
            g->hoff[g->hoffs++] = at;
            at += (size_t)sizes[f];
            if (heads[f].flags & 1) t->samples += heads[f].n;
        }
        g->hoff[g->hoffs++] = at;
    }
    g->hframes += total;
    g->hused += bytes;
    g->hup_add += (long long)bytes + (long long)((nr + 1) * sizeof(int64_t));
    free(w);
    return total;
}

FLAKE_AMD_API long long flake_amd_decode_set_held_windows(FlakeAmdDecodeSet *g, int nwin, const int *held_of_win,
        const unsigned long long *first_sample, const long long *count, void *pcm, int sample_bytes, size_t pcm_cap_samples,
        long long *win_samples, int *win_status, long long *frames_decoded)
{
    static const int none = 0;
    if (g && nwin > 0 && !held_of_win) { snprintf(g->err, sizeof g->err, "bad argument"); return -1; }
    const ds_win_call q = {nwin, NULL, NULL, 0, NULL, NULL, first_sample, count, pcm, sample_bytes, pcm_cap_samples, NULL,
                           win_samples, win_status, held_of_win ? held_of_win : &none};
    return ds_windows(g, &q, frames_decoded);
}

FLAKE_AMD_API long long flake_amd_decode_set_held_windows_rows(FlakeAmdDecodeSet *g, int nwin, const int *held_of_win,
        const unsigned long long *first_sample, const long long *count, void *dev_rows, int row_format, long long row_len,
        long long *win_samples, int *win_status, long long *frames_decoded)
{
    static const int none = 0;
    if (g && nwin > 0 && !held_of_win) { snprintf(g->err, sizeof g->err, "bad argument"); return -1; }
    const ds_rows_sink sink = {dev_rows, row_format, row_len, 0, 0, NULL, NULL};
    const ds_win_call q = {nwin, NULL, NULL, 0, NULL, NULL, first_sample, count, NULL, 4, 0, &sink, win_samples, win_status,
                           held_of_win ? held_of_win : &none};
    return ds_windows(g, &q, frames_decoded);
}

FLAKE_AMD_API long long flake_amd_span_rows_count(long long count, long long row_len, long long hop)
{
    return fa_sr_count(count, row_len, hop);
}

FLAKE_AMD_API long long flake_amd_decode_set_span_rows(FlakeAmdDecodeSet *g, int nspans, const int *frames_of_span,
        const unsigned char *stream, size_t bytes, const int *frame_sizes,
        const unsigned *fixed_block_size, const unsigned long long *first_sample, const long long *count, long long hop,
        void *dev_rows, int row_format, long long row_len, long long rows_cap,
        int *span_first_row, long long *row_samples, int *span_status, long long *frames_decoded)
{
    if (g && hop < 1) { snprintf(g->err, sizeof g->err, "hop must be 1 .. 2^31 - 1"); return -1; }
    const ds_rows_sink sink = {dev_rows, row_format, row_len, hop, rows_cap, span_first_row, row_samples};
    const ds_win_call q = {nspans, frames_of_span, stream, bytes, frame_sizes, fixed_block_size, first_sample, count, NULL, 4, 0,
                           &sink, NULL, span_status, NULL};
    return ds_windows(g, &q, frames_decoded);
}

FLAKE_AMD_API long long flake_amd_decode_set_held_span_rows(FlakeAmdDecodeSet *g, int nspans, const int *held_of_span,
        const unsigned long long *first_sample, const long long *count, long long hop,
        void *dev_rows, int row_format, long long row_len, long long rows_cap,
        int *span_first_row, long long *row_samples, int *span_status, long long *frames_decoded)
{
    static const int none = 0;
    if (g && (hop < 1 || (nspans > 0 && !held_of_span))) {
        snprintf(g->err, sizeof g->err, "%s", hop < 1 ? "hop must be 1 .. 2^31 - 1" : "bad argument");
        return -1;
    }
    const ds_rows_sink sink = {dev_rows, row_format, row_len, hop, rows_cap, span_first_row, row_samples};
    const ds_win_call q = {nspans, NULL, NULL, 0, NULL, NULL, first_sample, count, NULL, 4, 0, &sink, NULL, span_status,
                           held_of_span ? held_of_span : &none};
    return ds_windows(g, &q, frames_decoded);
}

FLAKE_AMD_API int flake_amd_decode_set_held_info(const FlakeAmdDecodeSet *g, int id, long long *frames, long long *samples,
                                                 long long *bytes)
{
    if (!g || id < 0 || id >= g->hn) return -1;
    const fa_held_stream *t = &g->hs[id];
    if (frames) *frames = t->frames;
    if (samples) *samples = t->samples;
    if (bytes) *bytes = (long long)(g->hoff[t->off0 + t->frames] - g->hoff[t->off0]);
    return 0;
}

FLAKE_AMD_API int flake_amd_decode_set_held_stats(const FlakeAmdDecodeSet *g, long long out[4])
{
    if (!g || !out) return -1;
    out[0] = (long long)g->hused;
    out[1] = g->hframes;
    out[2] = g->hup_add;
    out[3] = g->hup_win;
    return 0;
}

FLAKE_AMD_API int flake_amd_decode_set_index(FlakeAmdDecodeSet *g, unsigned max_block_size, const unsigned char *stream,
                                             const size_t *range_first, int nranges, int *frame_sizes, int cap,
                                             long long *range_frames, size_t *range_consumed)
{
    if (!g) return -1;
    g->err[0] = 0;
    const int rc = fa_index_ranges(g->hip, max_block_size, stream, range_first, nranges, frame_sizes, cap,
                                   range_frames, range_consumed, g->err, sizeof g->err);
    if (rc == -1) snprintf(g->err, sizeof g->err, "bad argument");
    return rc;
}

FLAKE_AMD_API const char *flake_amd_decode_set_last_error(const FlakeAmdDecodeSet *g)
{
    return g ? g->err : g_open_err;
}

FLAKE_AMD_API void flake_amd_decode_set_close(FlakeAmdDecodeSet *g)
{
    if (!g) return;
    if (g->hip) { (void)fhip_sync(g->hip); fhip_destroy(g->hip); }
    if (g->states) fhip_device_free(g->states);
    if (g->hstore) fhip_device_free(g->hstore);
    free(g->hs); free(g->hsize); free(g->hhead); free(g->hoff);
    free(g->tables); free(g->wtables); free(g->run_off); free(g->foff); free(g->wstage);
    free(g);
}
