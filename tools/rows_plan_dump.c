/*
 * rows_plan_dump.c -- runs the encode-rows planner (flake_amd/host/rows_plan.h) on a case read from standard input and
 * prints its tables.  For tests/test_rows_plan_cpu.py, which builds it plain and with the sanitizers; every array is
 * allocated exactly as large as the planner's header promises.
 *
 * Input, whitespace-separated integers:
 *   nrows block nwslices nsslices
 *   nrows    x (len stream)
 *   nwslices x (lo hi)                     parts of the whole table's destination, ascending
 *   nsslices x (lo hi)                     parts of the short table's destination, ascending
 * Output:
 *   "E -1" where fa_rows_count refuses; else "N nwhole nwhole_pieces nshort", "W streams...", "P row count col dst" per
 *   whole piece, "F first..." (every row's first whole block and the total), "Z size stream row" per short block,
 *   "S row count col dst" per short piece, then per slice "L count" and its "Q" pieces (whole) and "M count" and its
 *   "R" pieces (short).
 */
#include <stdio.h>
#include <stdlib.h>

#include "rows_plan.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

static void piece(const char *tag, const fhip_row_piece *q)
{
    printf("%s %d %d %lld %lld\n", tag, q->row, q->count, (long long)q->col, (long long)q->dst);
}

static void slices(int nslices, const fhip_row_piece *tab, int n, const char *head, const char *tag)
{
    fhip_row_piece *part = (fhip_row_piece *)malloc((size_t)n * sizeof(fhip_row_piece));
    int cur = 0;
    for (int i = 0; i < nslices; i++) {
        const long long lo = rd(), hi = rd();
        const int m = fa_rows_slice(tab, n, &cur, lo, hi, part);
        printf("%s %d\n", head, m);
        for (int j = 0; j < m; j++) piece(tag, &part[j]);
    }
    free(part);
}

int main(void)
{
    const int nrows = (int)rd(), block = (int)rd(), nwslices = (int)rd(), nsslices = (int)rd();
    const size_t nr = (size_t)nrows;
    long long *len = (long long *)malloc(nr * sizeof(long long));
    int *stream = (int *)malloc(nr * sizeof(int));
    for (int r = 0; r < nrows; r++) { len[r] = rd(); stream[r] = (int)rd(); }
    fa_rows_counts n;
    if (fa_rows_count(nrows, len, block, &n) != 0) {
        printf("E -1\n");
        free(len); free(stream);
        return 0;
    }
    int32_t *whole_stream = (int32_t *)malloc((size_t)n.nwhole * sizeof(int32_t));
    fhip_row_piece *whole_pieces = (fhip_row_piece *)malloc((size_t)n.nwhole_pieces * sizeof(fhip_row_piece));
    int32_t *short_size = (int32_t *)malloc((size_t)n.nshort * sizeof(int32_t));
    int32_t *short_stream = (int32_t *)malloc((size_t)n.nshort * sizeof(int32_t));
    int32_t *short_row = (int32_t *)malloc((size_t)n.nshort * sizeof(int32_t));
    fhip_row_piece *short_pieces = (fhip_row_piece *)malloc((size_t)n.nshort * sizeof(fhip_row_piece));
    int32_t *first = (int32_t *)malloc((nr + 1) * sizeof(int32_t));
    fa_rows_plan(nrows, len, stream, block, whole_stream, whole_pieces, short_size, short_stream, short_pieces, first,
                 short_row);
    printf("N %d %d %d\n", n.nwhole, n.nwhole_pieces, n.nshort);
    printf("W");
    for (int b = 0; b < n.nwhole; b++) printf(" %d", whole_stream[b]);
    printf("\n");
    for (int i = 0; i < n.nwhole_pieces; i++) piece("P", &whole_pieces[i]);
    printf("F");
    for (int r = 0; r <= nrows; r++) printf(" %d", first[r]);
    printf("\n");
    for (int i = 0; i < n.nshort; i++) printf("Z %d %d %d\n", short_size[i], short_stream[i], short_row[i]);
    for (int i = 0; i < n.nshort; i++) piece("S", &short_pieces[i]);
    slices(nwslices, whole_pieces, n.nwhole_pieces, "L", "Q");
    slices(nsslices, short_pieces, n.nshort, "M", "R");
    free(whole_stream); free(whole_pieces); free(short_size); free(short_stream); free(short_row); free(short_pieces);
    free(first); free(len); free(stream);
    return 0;
}
