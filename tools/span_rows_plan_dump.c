/*
 * span_rows_plan_dump.c -- flake_amd/host/span_rows_plan.h on cases read from standard input, its tables printed:
 * what tests/test_span_rows_plan_cpu.py holds against a Python model, plain and under the sanitizers.  Every table is
 * allocated at exactly the size the header asks for, so that a write past one is a report.
 *
 * A case is a line of numbers:
 *   row_len hop rows_cap nspans  (count delivered) x nspans  nsegs  (span, or -1) x nsegs
 * and prints
 *   C  fa_sr_count of every count
 *   F  fa_sr_first_rows' answer, and the table where it is not -1
 *   L  fa_sr_lengths' row_samples             (where F is not -1)
 *   B  fa_sr_batch's row0:nrows per segment   (likewise)
 *
 *   gcc -std=gnu99 -I flake_amd/host tools/span_rows_plan_dump.c -o span_rows_plan_dump
 */
#include <stdio.h>
#include <stdlib.h>

#include "span_rows_plan.h"

static long long next(void)
{
    long long v;
    if (scanf("%lld", &v) != 1) exit(3);
    return v;
}

int main(void)
{
    long long row_len;
    while (scanf("%lld", &row_len) == 1) {
        const long long hop = next(), rows_cap = next();
        const int nspans = (int)next();
        long long *count = malloc(sizeof *count * (size_t)(nspans ? nspans : 1));
        long long *delivered = malloc(sizeof *delivered * (size_t)(nspans ? nspans : 1));
        int32_t *first = malloc(sizeof *first * (size_t)(nspans + 1));
        if (!count || !delivered || !first) return 2;
        for (int s = 0; s < nspans; s++) { count[s] = next(); delivered[s] = next(); }
        const int nsegs = (int)next();
        int32_t *seg_row = malloc(sizeof *seg_row * (size_t)(nsegs ? nsegs : 1));
        int32_t *seg_nrows = malloc(sizeof *seg_nrows * (size_t)(nsegs ? nsegs : 1));
        if (!seg_row || !seg_nrows) return 2;
        for (int k = 0; k < nsegs; k++) seg_row[k] = (int32_t)next();
        printf("C");
        for (int s = 0; s < nspans; s++) printf(" %lld", fa_sr_count(count[s], row_len, hop));
        const long long total = fa_sr_first_rows(nspans, count, row_len, hop, rows_cap, first);
        printf("\nF %lld", total);
        if (total >= 0) {
            for (int s = 0; s <= nspans; s++) printf(" %d", first[s]);
            long long *row_samples = malloc(sizeof *row_samples * (size_t)(total ? total : 1));
            if (!row_samples) return 2;
            fa_sr_lengths(nspans, first, delivered, row_len, hop, row_samples);
            printf("\nL");
            for (long long r = 0; r < total; r++) printf(" %lld", row_samples[r]);
            fa_sr_batch(nsegs, first, seg_row, seg_nrows);
            printf("\nB");
            for (int k = 0; k < nsegs; k++) printf(" %d:%d", seg_row[k], seg_nrows[k]);
            free(row_samples);
        }
        printf("\n");
        free(count); free(delivered); free(first); free(seg_row); free(seg_nrows);
    }
    return 0;
}
