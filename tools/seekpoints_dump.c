/*
 * seekpoints_dump.c -- runs the seek-point recorder (flake_amd/host/seekpoints.h) on a sequence of blocks read from
 * standard input.  tests/test_seekpoints_cpu.py builds it with -fsanitize=address,undefined and holds its output to the
 * rule restated in Python.  No GPU, no HIP.
 *
 * Input (integers):  spacing nops   nops x { 0 samples bytes first_frame_samples | 1 | 2 }
 *                    0: one committed block, 1: save the recorder's state, 2: restore the state saved last
 * Output:  per point "P sample offset frame_samples", then "C samples bytes points": the counters at the end.
 */
#include <stdio.h>
#include <stdlib.h>

#include "seekpoints.h"

static unsigned long long rd(void)
{
    unsigned long long v = 0;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(void)
{
    fa_seekrec r = {0};
    fa_seekrec_mark mark;
    fa_seekrec_init(&r, rd());
    mark = fa_seekrec_save(&r);
    const unsigned long long nops = rd();
    for (unsigned long long i = 0; i < nops; i++) {
        const unsigned long long op = rd();
        if (op == 0) {
            const unsigned long long samples = rd(), bytes = rd();
            if (fa_seekrec_block(&r, samples, bytes, (unsigned)rd())) { fprintf(stderr, "out of memory\n"); return 1; }
        } else if (op == 1) {
            mark = fa_seekrec_save(&r);
        } else {
            fa_seekrec_restore(&r, &mark);
        }
    }
    FlakeAmdSeekPoint *pts = (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)(r.n ? r.n : 1));    /* exactly as many */
    const long long n = fa_seekrec_get(&r, pts, r.n);
    for (long long i = 0; i < n; i++) printf("P %llu %llu %u\n", pts[i].sample, pts[i].offset, pts[i].frame_samples);
    printf("C %llu %llu %lld\n", r.samples, r.bytes, n);
    free(pts);
    fa_seekrec_free(&r);
    return 0;
}
