/*
 * decode_set_plan_dump.c -- runs the decode set's batch planner (flake_amd/host/decode_set_plan.h) on a call read from
 * standard input and prints every table it makes.  tests/test_decode_set_plan_cpu.py holds the output to the expected
 * tables, built plain and with -fsanitize=address,undefined: every array here has exactly the size the planner is
 * promised, so an index one past it is reported.  No GPU, no HIP.
 *
 * Input (integers, any white space):  nstreams max_batch nruns nframes bytes
 *                                     nstreams x { started variable failed next_number samples_per_frame }
 *                                     nruns x { stream frames }      nframes x { size }
 * A negative nframes passes a null size table.  After each batch the streams are moved on as the set moves them when
 * every frame was good and held samples_per_frame samples: the numbering carry of the next batch is then visible.
 *
 * Output:  "E <code>" when fa_ds_check refuses the call, else per batch
 *          "B frame0 nframes nsegs byte0 nbytes", per segment "S first number variable stream run frame0 prev",
 *          "F" + seg_first, "M" + md5_first, "R" + md5_range; "T total_frames" at the end.
 */
#include <stdio.h>
#include <stdlib.h>

#include "decode_set_plan.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(void)
{
    const int nstreams = (int)rd(), max_batch = (int)rd(), nruns = (int)rd();
    const long long nframes = rd();
    const size_t bytes = (size_t)rd();
    const size_t ns = nstreams > 0 ? (size_t)nstreams : 0, nr = nruns > 0 ? (size_t)nruns : 0;
    const size_t nf = nframes > 0 ? (size_t)nframes : 0, mb = max_batch > 0 ? (size_t)max_batch : 0;
    fa_ds_stream *st = (fa_ds_stream *)malloc(sizeof *st * (ns ? ns : 1));
    long long *per = (long long *)malloc(sizeof *per * (ns ? ns : 1));
    int *sor = (int *)malloc(sizeof *sor * (nr ? nr : 1)), *fof = (int *)malloc(sizeof *fof * (nr ? nr : 1));
    int *sizes = (int *)malloc(sizeof *sizes * (nf ? nf : 1));
    for (size_t s = 0; s < ns; s++) {
        st[s].started = (int)rd(); st[s].variable = (int)rd(); st[s].failed = (int)rd();
        st[s].next_number = rd(); per[s] = rd();
        st[s].block = st[s].ended = 0;
    }
    for (size_t r = 0; r < nr; r++) { sor[r] = (int)rd(); fof[r] = (int)rd(); }
    for (size_t f = 0; f < nf; f++) sizes[f] = (int)rd();
    long long total = -1;
    const int rc = fa_ds_check(nstreams, st, nruns, sor, fof, nframes < 0 ? NULL : sizes, bytes, &total);
    if (rc != FA_DS_OK) {
        printf("E %d\n", rc);
        free(st); free(per); free(sor); free(fof); free(sizes);
        return 0;
    }
    fa_ds_batch b;
    b.seg_first = (int32_t *)malloc(sizeof(int32_t) * (mb + 1));
    b.seg_number = (int64_t *)malloc(sizeof(int64_t) * (mb ? mb : 1));
    b.seg_variable = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_stream = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_run = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_frame0 = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.seg_prev = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.md5_first = (int32_t *)malloc(sizeof(int32_t) * (ns + 1));
    b.md5_range = (int32_t *)malloc(sizeof(int32_t) * (mb ? mb : 1));
    b.last_seg = (int32_t *)malloc(sizeof(int32_t) * ns);
    b.planned = (long long *)malloc(sizeof(long long) * ns);
    fa_ds_cursor cur = {0, 0, 0, 0};
    while (fa_ds_plan(&cur, nruns, sor, fof, sizes, nstreams, st, max_batch, &b) > 0) {
        printf("B %lld %d %d %zu %zu\n", b.frame0, b.nframes, b.nsegs, b.byte0, b.nbytes);
        for (int k = 0; k < b.nsegs; k++)
            printf("S %d %lld %d %d %d %d %d\n", b.seg_first[k], (long long)b.seg_number[k], b.seg_variable[k],
                   b.seg_stream[k], b.seg_run[k], b.seg_frame0[k], b.seg_prev[k]);
        printf("F");
        for (int k = 0; k <= b.nsegs; k++) printf(" %d", b.seg_first[k]);
        printf("\nM");
        for (int s = 0; s <= nstreams; s++) printf(" %d", b.md5_first[s]);
        printf("\nR");
        for (int k = 0; k < b.nsegs; k++) printf(" %d", b.md5_range[k]);
        printf("\n");
        for (int k = 0; k < b.nsegs; k++) {
            fa_ds_stream *t = &st[b.seg_stream[k]];
            const int n = b.seg_first[k + 1] - b.seg_first[k];
            if (t->started && !t->failed) t->next_number += t->variable ? n * per[b.seg_stream[k]] : n;
        }
    }
    printf("T %lld\n", total);
    free(b.seg_first); free(b.seg_number); free(b.seg_variable); free(b.seg_stream); free(b.seg_run); free(b.seg_frame0);
    free(b.seg_prev); free(b.md5_first); free(b.md5_range); free(b.last_seg); free(b.planned);
    free(st); free(per); free(sor); free(fof); free(sizes);
    return 0;
}
