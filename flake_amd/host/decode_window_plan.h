/*
 * decode_window_plan.h -- the planner of flake_amd_decode_set_windows (flake_decode_set.c): which frames of a run cover a
 * window of samples, what the device must drop and deliver of them (fhip_decode_frames_windows' seg_skip / seg_take),
 * and how the selected frames of a call are cut into device batches.  Plain C on plain tables: no call into the HIP
 * layer, so that it is tested and run under the sanitizers on the CPU (tests/test_decode_window_plan_cpu.py).  The
 * sibling of decode_set_plan.h and recode_plan.h.
 *
 * A RUN is consecutive frames of one stream, back to back with their sizes, starting at any frame of the stream.  A frame's
 * first sample follows from its header alone: the coded number itself in a variable-block-size stream (bit 15), the number
 * times the stream's fixed block size otherwise -- STREAMINFO's where minimum and maximum agree, else (0) the size of the
 * run's first frame.  The numbers increase along a run, so the frames that overlap a window are found by bisection: the
 * planner reads the run's first header, the headers it probes, and nothing else.  It trusts no header beyond that: the
 * device decodes and checks every selected frame, its numbering held from the number the planner names.
 *
 * Where a header comes from is an ACCESSOR's business (fa_dw_headers: "the header of frame k of window w's run"): the one
 * here parses it out of the run's bytes, held_plan.h's reads it out of the table the device left when the stream was
 * taken into a held store.  fa_dw_select_by / fa_dw_plan_by are the one selection and the one batch rule over either;
 * fa_dw_select / fa_dw_plan are those over the bytes.
 * Not installed.
 */
#ifndef FLAKE_AMD_DECODE_WINDOW_PLAN_H
#define FLAKE_AMD_DECODE_WINDOW_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "../csrc/flac_header.h"

enum { FA_DW_OK = 0,              /* frames were selected */
       FA_DW_EMPTY = 1,           /* nothing to decode: the window delivers 0 */
       FA_DW_FAILED_HEADER = -1   /* a header the search needed is not a header of this stream */ };

/* What fa_dw_select found for one window.  Frames are counted from the run's first, bytes from wherever off[] counts. */
typedef struct fa_dw_sel {
    int status;
    int frame0, nframes;          /* the sub-run: the frames that overlap the window */
    size_t byte0, nbytes;         /* its bytes: off[frame0] .. off[frame0 + nframes] */
    long long number;             /* the number its first frame carries: the segment's seg_number */
    int variable;                 /* the blocking-strategy bit */
    long long skip, take;         /* samples to drop from the sub-run's front, and the most to deliver behind them */
    long long deliver;            /* what a stream whose numbers do not lie delivers: take, cut at the run's end */
    long long start;              /* the first sample of the sub-run's first frame */
    int block;                    /* fixed blocks: the size a frame number is multiplied by */
} fa_dw_sel;

/* The header of frame k of window w's run: 1 and *h where it is one of this stream, else 0. */
typedef struct fa_dw_headers {
    int (*get)(const void *ctx, int w, int k, flac_header *h);
    const void *ctx;
} fa_dw_headers;

/* The accessor over the runs' bytes: run_data[w] / run_sizes[w] / run_off[w] are window w's run. */
typedef struct fa_dw_bytes {
    const flac_format *fmt;
    const unsigned char *const *run_data;
    const int *const *run_sizes;
    const size_t *const *run_off;
} fa_dw_bytes;

static inline int fa_dw_bytes_get(const void *ctx, int w, int k, flac_header *h)
{
    const fa_dw_bytes *b = (const fa_dw_bytes *)ctx;
    return flac_header_ok(b->fmt, b->run_data[w] + b->run_off[w][k], b->run_sizes[w][k], h);
}

static inline long long fa_dw_start(const flac_header *h, int block)
{
    return h->vbs ? (long long)h->number : (long long)h->number * block;
}

/* Select the frames of window w's run that overlap [first_sample, first_sample + count).  hd answers for the run's
 * headers; off [nframes + 1] (off[k] = where frame k begins, off[nframes] = the run's end) are its bytes; count >= 0. */
static inline int fa_dw_select_by(const fa_dw_headers *hd, int w, const size_t *off, int nframes, unsigned fixed_block_size,
                                  unsigned long long first_sample, long long count, fa_dw_sel *o)
{
    flac_header h0, ha, hb;
    o->status = FA_DW_EMPTY;
    o->frame0 = o->nframes = 0;
    o->byte0 = o->nbytes = 0;
    o->number = -1;
    o->variable = 0;
    o->skip = o->take = o->deliver = o->start = 0;
    o->block = 0;
    if (count <= 0 || nframes <= 0) return o->status;
    if (first_sample > 0x7FFFFFFFFFFFFFFFull - (unsigned long long)count) return o->status;    /* behind any stream's end */
    if (!hd->get(hd->ctx, w, 0, &h0)) return o->status = FA_DW_FAILED_HEADER;
    const int block = h0.vbs ? 0 : (fixed_block_size ? (int)fixed_block_size : h0.n);
    const long long first = (long long)first_sample, end = first + count;
    if (first < fa_dw_start(&h0, block)) return o->status;              /* begins before the run's first frame */
    /* a: the last frame that starts at or before the window */
    int lo = 0, hi = nframes - 1;
    ha = h0;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        flac_header h;
        if (!hd->get(hd->ctx, w, mid, &h)) return o->status = FA_DW_FAILED_HEADER;
        if (fa_dw_start(&h, block) <= first) { lo = mid; ha = h; } else hi = mid - 1;
    }
    const int a = lo;
    const long long start_a = fa_dw_start(&ha, block);
    if (a == nframes - 1 && first >= start_a + ha.n) return o->status;  /* at or behind the run's end */
    /* b: the last frame that starts before the window's end */
    lo = a;
    hi = nframes - 1;
    hb = ha;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        flac_header h;
        if (!hd->get(hd->ctx, w, mid, &h)) return o->status = FA_DW_FAILED_HEADER;
        if (fa_dw_start(&h, block) < end) { lo = mid; hb = h; } else hi = mid - 1;
    }
    const int b = lo;
    const long long run_end = fa_dw_start(&hb, block) + hb.n;
    o->status = FA_DW_OK;
    o->frame0 = a;
    o->nframes = b - a + 1;
    o->byte0 = off[a];
    o->nbytes = off[b + 1] - off[a];
    o->number = (long long)ha.number;
    o->variable = ha.vbs;
    o->skip = first - start_a;
    o->take = count;
    o->deliver = run_end > first ? (end < run_end ? count : run_end - first) : 0;
    o->start = start_a;
    o->block = block;
    return o->status;
}

/* The same over the run's bytes: sizes [nframes] and off describe the run in data. */
static inline int fa_dw_select(const flac_format *fmt, const unsigned char *data, const int *sizes, const size_t *off,
                               int nframes, unsigned fixed_block_size, unsigned long long first_sample, long long count,
                               fa_dw_sel *o)
{
    const fa_dw_bytes by = {fmt, &data, &sizes, &off};
    const fa_dw_headers hd = {fa_dw_bytes_get, &by};
    return fa_dw_select_by(&hd, 0, off, nframes, fixed_block_size, first_sample, count, o);
}

/* ---- batches --------------------------------------------------------------------------------------------------------
 * The selected sub-runs of a call, in call order, cut into device batches of at most max_batch frames at frame boundaries.
 * The part of a sub-run inside a batch is one SEGMENT.  A cut may fall inside a window: the part behind it is numbered by
 * the header at the cut, which says how many samples lie before it, and skip and take carry over -- what is left to drop,
 * what is left to deliver.  Should that header not be one, the window becomes FA_DW_FAILED_HEADER as a whole and the
 * part in front of the cut is not planned either. */
typedef struct fa_dw_cursor {
    int win, taken;               /* the next window, and how many frames of its sub-run are planned already */
    long long start;              /* the first sample of the frame the next part begins with (taken > 0) */
    long long number;             /* ... and the number it carries */
    long long skip, take;         /* what is left of the window's skip and take (taken > 0) */
} fa_dw_cursor;

/* One batch.  The arrays are the caller's: seg_first [max_batch + 1], every other one [max_batch]. */
typedef struct fa_dw_batch {
    int nframes, nsegs;
    size_t nbytes;
    int32_t *seg_first;           /* CSR over the batch's frames */
    int64_t *seg_number;
    int32_t *seg_variable;
    int64_t *seg_skip, *seg_take;
    int32_t *seg_win;             /* the window the segment is a part of */
    int32_t *seg_frame0;          /* its first frame, counted from the window's run's first */
    int32_t *seg_last;            /* 1: the window's last part */
} fa_dw_batch;

/* The next batch: fills *b from *cur (all zero before the first) and moves *cur behind it.  sel [nwin] are the windows'
 * selections; hd and run_off[w] are window w's run as fa_dw_select_by took it.
 * Returns the batch's frames; 0 when the call is used up. */
static inline int fa_dw_plan_by(fa_dw_cursor *cur, int nwin, fa_dw_sel *sel, const fa_dw_headers *hd,
                                const size_t *const *run_off, int max_batch, fa_dw_batch *b)
{
    b->nframes = b->nsegs = 0;
    b->nbytes = 0;
    b->seg_first[0] = 0;
    while (cur->win < nwin && b->nframes < max_batch) {
        const int w = cur->win;
        fa_dw_sel *s = &sel[w];
        if (s->status != FA_DW_OK || cur->taken >= s->nframes) { cur->win++; cur->taken = 0; continue; }
        if (cur->taken == 0) { cur->start = s->start; cur->number = s->number; cur->skip = s->skip; cur->take = s->take; }
        const int left = s->nframes - cur->taken, room = max_batch - b->nframes, take = left < room ? left : room;
        const int f0 = s->frame0 + cur->taken;
        long long next_start = 0, next_number = 0;
        if (take < left) {
            /* a cut inside the window: the header behind it says where the next part begins */
            flac_header h;
            const int f = f0 + take;
            if (!hd->get(hd->ctx, w, f, &h) || h.vbs != s->variable ||
                fa_dw_start(&h, s->block) <= cur->start) {
                /* the whole window fails: its earlier parts' results are the caller's to drop */
                s->status = FA_DW_FAILED_HEADER;
                cur->win++;
                cur->taken = 0;
                continue;
            }
            next_start = fa_dw_start(&h, s->block);
            next_number = (long long)h.number;
        }
        const int k = b->nsegs++;
        b->seg_number[k] = cur->number;
        b->seg_variable[k] = s->variable;
        b->seg_skip[k] = cur->skip;
        b->seg_take[k] = cur->take;
        b->seg_win[k] = w;
        b->seg_frame0[k] = f0;
        b->seg_last[k] = take == left;
        b->nbytes += run_off[w][f0 + take] - run_off[w][f0];
        b->nframes += take;
        b->seg_first[k + 1] = b->nframes;
        if (take < left) {
            const long long part = next_start - cur->start;             /* the samples of this part's frames */
            const long long got = part > cur->skip ? (part - cur->skip < cur->take ? part - cur->skip : cur->take) : 0;
            cur->skip = cur->skip > part ? cur->skip - part : 0;
            cur->take -= got;
            cur->start = next_start;
            cur->number = next_number;
            cur->taken += take;
        } else {
            cur->win++;
            cur->taken = 0;
        }
    }
    return b->nframes;
}

/* The same over the runs' bytes: run_data[w] / run_sizes[w] / run_off[w] are window w's run as fa_dw_select took it. */
static inline int fa_dw_plan(fa_dw_cursor *cur, int nwin, fa_dw_sel *sel, const flac_format *fmt,
                             const unsigned char *const *run_data, const int *const *run_sizes,
                             const size_t *const *run_off, int max_batch, fa_dw_batch *b)
{
    const fa_dw_bytes by = {fmt, run_data, run_sizes, run_off};
    const fa_dw_headers hd = {fa_dw_bytes_get, &by};
    return fa_dw_plan_by(cur, nwin, sel, &hd, run_off, max_batch, b);
}

#endif
