/*
 * decode_window_plan_dump.c -- runs the window planner (flake_amd/host/decode_window_plan.h) on a call read from
 * standard input and prints what it selects and every batch it cuts.  tests/test_decode_window_plan_cpu.py holds the
 * output to tables written out by hand, built plain and with -fsanitize=address,undefined: every array here has exactly
 * the size the planner is promised, and every run's bytes lie in a block of exactly their length, so an index or a read
 * one past either is reported.  No GPU, no HIP.
 *
 * Input (integers, any white space):  channels bps sample_rate max_block_size  max_batch  nwin
 *                                     nwin x { nframes fixed_block_size first_sample count
 *                                              nframes x { size }  bytes x { byte } }
 * Each window has a run of its own (the planner is told so: one size table and one offset table per window).
 *
 * Output:  per window "W status frame0 nframes byte0 nbytes number variable skip take deliver", then per batch
 *          "B nframes nsegs nbytes" and per segment "S first number variable skip take win frame0 last"; at the end
 *          "E" + every window's status as the batches left it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode_window_plan.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(void)
{
    flac_format fmt;
    fmt.channels = (int)rd(); fmt.bps = (int)rd(); fmt.sample_rate = (int)rd(); fmt.max_block_size = (int)rd();
    const int max_batch = (int)rd(), nwin = (int)rd();
    const size_t nw = nwin > 0 ? (size_t)nwin : 0, mb = max_batch > 0 ? (size_t)max_batch : 0;
    fa_dw_sel *sel = (fa_dw_sel *)malloc(sizeof *sel * (nw ? nw : 1));
    int **sizes = (int **)calloc(nw ? nw : 1, sizeof *sizes);
    size_t **off = (size_t **)calloc(nw ? nw : 1, sizeof *off);
    unsigned char **data = (unsigned char **)calloc(nw ? nw : 1, sizeof *data);
    for (size_t w = 0; w < nw; w++) {
        const int nf = (int)rd();
        const unsigned fixed = (unsigned)rd();
        const unsigned long long first = (unsigned long long)rd();
        const long long count = rd();
        sizes[w] = (int *)malloc(sizeof(int) * (size_t)(nf > 0 ? nf : 1));
        off[w] = (size_t *)malloc(sizeof(size_t) * ((size_t)(nf > 0 ? nf : 0) + 1));
        off[w][0] = 0;
        for (int f = 0; f < nf; f++) { sizes[w][f] = (int)rd(); off[w][f + 1] = off[w][f] + (size_t)sizes[w][f]; }
        const size_t bytes = off[w][nf > 0 ? nf : 0];
        data[w] = (unsigned char *)malloc(bytes ? bytes : 1);
        for (size_t i = 0; i < bytes; i++) data[w][i] = (unsigned char)rd();
        fa_dw_select(&fmt, data[w], sizes[w], off[w], nf, fixed, first, count, &sel[w]);
        printf("W %d %d %d %zu %zu %lld %d %lld %lld %lld\n", sel[w].status, sel[w].frame0, sel[w].nframes, sel[w].byte0,
               sel[w].nbytes, sel[w].number, sel[w].variable, sel[w].skip, sel[w].take, sel[w].deliver);
    }
    fa_dw_batch b;
    b.seg_first = (int32_t *)malloc(sizeof(int32_t) * (mb + 1));
    b.seg_number = (int64_t *)malloc(sizeof(int64_t) * (mb ? mb : 1));
    b.seg_variable = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_skip = (int64_t *)malloc(sizeof(int64_t) * (mb ? mb : 1));
    b.seg_take = (int64_t *)malloc(sizeof(int64_t) * (mb ? mb : 1));
    b.seg_win = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_frame0 = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_last = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    fa_dw_cursor cur;
    memset(&cur, 0, sizeof cur);
    while (fa_dw_plan(&cur, nwin, sel, &fmt, (const unsigned char *const *)data, (const int *const *)sizes,
                      (const size_t *const *)off, max_batch, &b) > 0) {
        printf("B %d %d %zu\n", b.nframes, b.nsegs, b.nbytes);
        for (int k = 0; k < b.nsegs; k++)
            printf("S %d %lld %d %lld %lld %d %d %d\n", b.seg_first[k], (long long)b.seg_number[k], b.seg_variable[k],
                   (long long)b.seg_skip[k], (long long)b.seg_take[k], b.seg_win[k], b.seg_frame0[k], b.seg_last[k]);
    }
    printf("E");
    for (size_t w = 0; w < nw; w++) printf(" %d", sel[w].status);
    printf("\n");
    free(b.seg_first); free(b.seg_number); free(b.seg_variable); free(b.seg_skip); free(b.seg_take); free(b.seg_win);
    free(b.seg_frame0); free(b.seg_last);
    for (size_t w = 0; w < nw; w++) { free(sizes[w]); free(off[w]); free(data[w]); }
    free(sizes); free(off); free(data); free(sel);
    return 0;
}
