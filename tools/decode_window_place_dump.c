/*
 * decode_window_place_dump.c -- runs the window placement (flake_amd/host/decode_window_place.h) on a call read from
 * standard input and prints where it puts every batch, every segment and every window.
 * tests/test_decode_window_place_cpu.py holds the output to tables written out by hand, built plain and with
 * -fsanitize=address,undefined: every table here has exactly the size the header is promised -- the windows' tables
 * nwin entries, a batch's tables as many as it has segments -- so an index one past any of them is reported.  No GPU, no
 * HIP, and no planner: the batches are given as the planner and the device would leave them.
 *
 * Input (integers, any white space):  rows nwin  nwin x { status count }  nbatches
 *                                     nbatches x { nchange  nchange x { window status }
 *                                                  nsegs  nsegs x { window last samples failed fail_status } }
 *                                     nchange  nchange x { window status }
 * status: a window's selection status (FA_DW_*); a change is the planner failing a window at a cut before it plans the
 * batch (or, the last list, finds nothing more to plan).  rows: 1 asks for the rows sink's tables.
 *
 * Output:  per batch "B base" and per segment "S target row col" (row and col 0 without rows); at the end per window
 *          "W at samples status" and "T total".
 */
#include <stdio.h>
#include <stdlib.h>

#include "decode_window_place.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

static void changes(fa_dw_sel *sel)
{
    for (int n = (int)rd(); n > 0; n--) {
        const int w = (int)rd();
        sel[w].status = (int)rd();
    }
}

int main(void)
{
    const int rows = (int)rd(), nwin = (int)rd();
    const size_t nw = (size_t)nwin;
    fa_dw_sel *sel = (fa_dw_sel *)calloc(nw, sizeof *sel);
    long long *count = (long long *)malloc(nw * sizeof *count), *win_at = (long long *)malloc(nw * sizeof *win_at);
    long long *win_samples = (long long *)malloc(nw * sizeof *win_samples);
    int *win_status = (int *)malloc(nw * sizeof *win_status);
    for (int w = 0; w < nwin; w++) { sel[w].status = (int)rd(); count[w] = rd(); }
    fa_wp_state st;
    fa_wp_begin(&st, nwin, sel, count, win_at, win_samples, win_status);
    for (int nb = (int)rd(); nb > 0; nb--) {
        changes(sel);
        const int nsegs = (int)rd();
        const size_t ns = (size_t)nsegs;
        int32_t *seg_win = (int32_t *)malloc(ns * sizeof(int32_t)), *seg_last = (int32_t *)malloc(ns * sizeof(int32_t));
        int32_t *seg_failed = (int32_t *)malloc(ns * sizeof(int32_t)), *seg_status = (int32_t *)malloc(ns * sizeof(int32_t));
        int32_t *seg_row = (int32_t *)calloc(ns, sizeof(int32_t));
        int64_t *seg_samples = (int64_t *)malloc(ns * sizeof(int64_t)), *seg_col = (int64_t *)calloc(ns, sizeof(int64_t));
        long long *seg_target = (long long *)malloc(ns * sizeof(long long));
        for (int k = 0; k < nsegs; k++) {
            seg_win[k] = (int32_t)rd(); seg_last[k] = (int32_t)rd(); seg_samples[k] = rd();
            seg_failed[k] = (int32_t)rd(); seg_status[k] = (int32_t)rd();
        }
        printf("B %lld\n", fa_wp_batch(&st, nsegs, seg_win, rows ? seg_row : NULL, rows ? seg_col : NULL));
        fa_wp_answers(&st, nsegs, seg_win, seg_last, seg_samples, seg_failed, seg_status, seg_target);
        for (int k = 0; k < nsegs; k++) printf("S %lld %d %lld\n", seg_target[k], seg_row[k], (long long)seg_col[k]);
        free(seg_win); free(seg_last); free(seg_failed); free(seg_status); free(seg_row); free(seg_samples); free(seg_col);
        free(seg_target);
    }
    changes(sel);
    const long long total = fa_wp_end(&st);
    for (int w = 0; w < nwin; w++) printf("W %lld %lld %d\n", win_at[w], win_samples[w], win_status[w]);
    printf("T %lld\n", total);
    free(sel); free(count); free(win_at); free(win_samples); free(win_status);
    return 0;
}
