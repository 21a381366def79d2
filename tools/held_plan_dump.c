/*
 * held_plan_dump.c -- runs the window planner twice on a call read from standard input: over the runs' bytes
 * (decode_window_plan.h's accessor) and over the table of heads a held store keeps (flake_amd/host/held_plan.h's), and
 * prints what each selects and every batch each cuts, the first under "bytes", the second under "table".
 * tests/test_held_plan_cpu.py holds the two halves to each other, built plain and with -fsanitize=address,undefined:
 * every array here has exactly the size the planner is promised, the heads of all runs lie back to back in one table of
 * exactly their number, and the table leg is given NO bytes at all, so a read of either that the accessor should not
 * make is reported.  No GPU, no HIP.
 *
 * Input (integers, any white space):  channels bps sample_rate max_block_size  max_batch  nwin
 *                                     nwin x { nframes fixed_block_size first_sample count
 *                                              nframes x { size }  bytes x { byte } }
 * Output, per leg:  "L bytes" or "L table", then decode_window_plan_dump.c's lines.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "held_plan.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

static void leg(const char *name, const fa_dw_headers *hd, int nwin, size_t **off, const int *nframes, const unsigned *fixed,
                const unsigned long long *first, const long long *count, int max_batch)
{
    const size_t nw = nwin > 0 ? (size_t)nwin : 0, mb = max_batch > 0 ? (size_t)max_batch : 0;
    fa_dw_sel *sel = (fa_dw_sel *)malloc(sizeof *sel * (nw ? nw : 1));
    printf("L %s\n", name);
    for (size_t w = 0; w < nw; w++) {
        fa_dw_select_by(hd, (int)w, off[w], nframes[w], fixed[w], first[w], count[w], &sel[w]);
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
    while (fa_dw_plan_by(&cur, nwin, sel, hd, (const size_t *const *)off, max_batch, &b) > 0) {
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
    free(sel);
}

int main(void)
{
    flac_format fmt;
    fmt.channels = (int)rd(); fmt.bps = (int)rd(); fmt.sample_rate = (int)rd(); fmt.max_block_size = (int)rd();
    const int max_batch = (int)rd(), nwin = (int)rd();
    const size_t nw = nwin > 0 ? (size_t)nwin : 0, n1 = nw ? nw : 1;
    int **sizes = (int **)calloc(n1, sizeof *sizes);
    size_t **off = (size_t **)calloc(n1, sizeof *off);
    unsigned char **data = (unsigned char **)calloc(n1, sizeof *data);
    int *nframes = (int *)calloc(n1, sizeof *nframes);
    unsigned *fixed = (unsigned *)calloc(n1, sizeof *fixed);
    unsigned long long *first = (unsigned long long *)calloc(n1, sizeof *first);
    long long *count = (long long *)calloc(n1, sizeof *count);
    long long *rec0 = (long long *)calloc(n1, sizeof *rec0);
    long long total = 0;
    for (size_t w = 0; w < nw; w++) {
        const int nf = (int)rd();
        nframes[w] = nf;
        fixed[w] = (unsigned)rd();
        first[w] = (unsigned long long)rd();
        count[w] = rd();
        sizes[w] = (int *)malloc(sizeof(int) * (size_t)(nf > 0 ? nf : 1));
        off[w] = (size_t *)malloc(sizeof(size_t) * ((size_t)(nf > 0 ? nf : 0) + 1));
        off[w][0] = 0;
        for (int f = 0; f < nf; f++) { sizes[w][f] = (int)rd(); off[w][f + 1] = off[w][f] + (size_t)sizes[w][f]; }
        const size_t bytes = off[w][nf > 0 ? nf : 0];
        data[w] = (unsigned char *)malloc(bytes ? bytes : 1);
        for (size_t i = 0; i < bytes; i++) data[w][i] = (unsigned char)rd();
        rec0[w] = total;
        total += nf > 0 ? nf : 0;
    }
    /* the table, as k_frame_heads leaves it: every frame's header through the one predicate */
    fa_held_head *heads = (fa_held_head *)malloc(sizeof *heads * (size_t)(total ? total : 1));
    for (size_t w = 0; w < nw; w++)
        for (int f = 0; f < nframes[w]; f++) {
            flac_header h;
            const int ok = flac_header_ok(&fmt, data[w] + off[w][f], sizes[w][f], &h);
            heads[rec0[w] + f] = fa_held_head_of(ok, &h);
        }
    const fa_dw_bytes by = {&fmt, (const unsigned char *const *)data, (const int *const *)sizes, (const size_t *const *)off};
    const fa_dw_headers hb = {fa_dw_bytes_get, &by};
    leg("bytes", &hb, nwin, off, nframes, fixed, first, count, max_batch);
    /* the table leg sees no byte of any run */
    for (size_t w = 0; w < nw; w++) { free(data[w]); data[w] = NULL; free(sizes[w]); sizes[w] = NULL; }
    const fa_held_table tab = {heads, rec0};
    const fa_dw_headers ht = {fa_held_get, &tab};
    leg("table", &ht, nwin, off, nframes, fixed, first, count, max_batch);
    for (size_t w = 0; w < nw; w++) free(off[w]);
    free(sizes); free(off); free(data); free(nframes); free(fixed); free(first); free(count); free(rec0); free(heads);
    return 0;
}
