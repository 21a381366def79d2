/*
 * decode_window_place.h -- where the samples of flake_amd_decode_set_windows' windows land in the call's output
 * (flake_decode_set.c), batch by batch as the device's answers come in, and what each window has delivered and whether
 * it failed.  Plain C on plain tables: no call into the HIP layer, so that it is tested and run under the sanitizers on
 * the CPU (tests/test_decode_window_place_cpu.py).  The sibling of decode_window_plan.h, whose selections and batches it
 * reads.  Not installed.
 *
 * THE RULE.  The windows lie in the output in call order, each behind the room of the one before it:
 *   - A window takes its place -- where the output has got to -- when the first of its segments, or of any later
 *     window's, is reached.
 *   - A window that failed, in the planner (FA_DW_FAILED_HEADER) or on the device in any of its segments, delivers
 *     nothing (win_samples -1) and keeps exactly count samples of room from where it began: the next window begins there.
 *   - A window that delivers nothing and did not fail keeps no room.
 *   - A good window's segments follow one another from where it began, and the next window begins behind the last.
 * The device writes a batch's clips back to back from where the output had got to when the batch was sent (fa_wp_batch);
 * a segment's TARGET is where the rule wants its samples, never before where the device put them.
 */
#ifndef FLAKE_AMD_DECODE_WINDOW_PLACE_H
#define FLAKE_AMD_DECODE_WINDOW_PLACE_H

#include "decode_window_plan.h"

/* The call's state.  The tables are the caller's, nwin entries each; sel and count are only read (sel at every step: the
 * planner may fail a window at a cut while the call is under way). */
typedef struct fa_wp_state {
    int nwin;
    const fa_dw_sel *sel;
    const long long *count;       /* what each window asked for */
    long long *win_at;            /* where the window's samples begin; -1: it has not taken its place */
    long long *win_samples;       /* what it has delivered; at the end -1 for a failed one */
    int *win_status;              /* 0, or why it failed: FA_WP_HEADER from the planner, the failing frame's status */
    long long out_at;             /* where the output has got to */
    int settled;                  /* the windows before this one have their place, their count and their room */
} fa_wp_state;

enum { FA_WP_HEADER = 1 };        /* (FHIP_VERIFY_HEADER: a window that failed in the planner) */

static inline void fa_wp_begin(fa_wp_state *st, int nwin, const fa_dw_sel *sel, const long long *count, long long *win_at,
                               long long *win_samples, int *win_status)
{
    st->nwin = nwin; st->sel = sel; st->count = count;
    st->win_at = win_at; st->win_samples = win_samples; st->win_status = win_status;
    st->out_at = 0;
    st->settled = 0;
    for (int w = 0; w < nwin; w++) { win_at[w] = -1; win_samples[w] = 0; win_status[w] = 0; }
}

/* THE settle step: the windows before `upto` that are not settled yet take their place, and a failed one its room. */
static inline void fa_wp_settle(fa_wp_state *st, int upto)
{
    for (; st->settled < upto; st->settled++) {
        const int w = st->settled;
        if (st->win_at[w] < 0) st->win_at[w] = st->out_at;
        if (!st->win_status[w] && st->sel[w].status == FA_DW_FAILED_HEADER) st->win_status[w] = FA_WP_HEADER;
        if (st->win_status[w]) st->out_at = st->win_at[w] + st->count[w];
    }
}

/* Before a batch is sent: settles the windows before its first segment's and returns where the device is to write the
 * batch's clips.  seg_row / seg_col (the rows sink; both or neither, nsegs entries): the segment's window as its row,
 * -1 for a window that has failed already, and what the window has delivered so far as its first column. */
static inline long long fa_wp_batch(fa_wp_state *st, int nsegs, const int32_t *seg_win, int32_t *seg_row, int64_t *seg_col)
{
    if (nsegs > 0) fa_wp_settle(st, seg_win[0]);
    for (int k = 0; k < nsegs && seg_row; k++) {
        const int w = seg_win[k];
        seg_row[k] = st->win_status[w] ? -1 : w;
        seg_col[k] = st->win_samples[w];
    }
    return st->out_at;
}

/* The batch's answers: seg_samples [nsegs] and seg_failed [nsegs] as the device left them, seg_status [nsegs] the failing
 * frame's status where seg_failed is not negative.  Leaves seg_target [nsegs]: where the segment's samples belong in
 * the output, -1 where they are dropped (a failed window's). */
static inline void fa_wp_answers(fa_wp_state *st, int nsegs, const int32_t *seg_win, const int32_t *seg_last,
                                 const int64_t *seg_samples, const int32_t *seg_failed, const int32_t *seg_status,
                                 long long *seg_target)
{
    for (int k = 0; k < nsegs; k++) {
        const int w = seg_win[k];
        fa_wp_settle(st, w);
        if (st->win_at[w] < 0) st->win_at[w] = st->out_at;
        if (!st->win_status[w] && seg_failed[k] >= 0) st->win_status[w] = seg_status[k];
        if (!st->win_status[w] && st->sel[w].status == FA_DW_FAILED_HEADER) st->win_status[w] = FA_WP_HEADER;
        seg_target[k] = st->win_status[w] ? -1 : st->out_at;
        if (!st->win_status[w]) {
            st->win_samples[w] += seg_samples[k];
            st->out_at += seg_samples[k];
        }
        if (seg_last[k]) fa_wp_settle(st, w + 1);
    }
}

/* After the last batch: settles what is left and returns what the good windows delivered. */
static inline long long fa_wp_end(fa_wp_state *st)
{
    long long total = 0;
    fa_wp_settle(st, st->nwin);
    for (int w = 0; w < st->nwin; w++) {
        if (st->win_status[w]) st->win_samples[w] = -1;
        else total += st->win_samples[w];
    }
    return total;
}

#endif
