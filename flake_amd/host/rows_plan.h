/*
 * rows_plan.h -- the planner of flake_amd_set_encode_rows (flake_set.c): how the rows of a padded planar batch on the
 * device become the blocks of a stream set's two calls -- as the piece tables K12 (fhip_pcm_from_rows_dev,
 * fhip_frames_packed_from_rows) takes.  Plain C on plain tables: no call into the HIP layer, so that it is tested and
 * run under the sanitizers on the CPU (tests/test_rows_plan_cpu.py).  The sibling of recode_plan.h.
 *
 * Row r holds len_of_row[r] samples (0 .. row_len, the caller has checked) of stream stream_of_row[r] and is cut into
 * len / B whole blocks and, where len % B != 0, one short block of len % B samples.  Two tables:
 *   whole   every row's whole blocks in (row, block) order, with whole_stream[] naming each block's stream, and ONE
 *           piece per row that has any (a piece spans the row's whole run of blocks: (len / B) * B samples from
 *           column 0).  The pieces tile [0, nwhole * B).
 *   short   one block per row with len % B != 0, in row order, with short_size[], short_stream[] and one piece each
 *           (len % B samples from column (len / B) * B).  The pieces tile [0, the sum of the sizes).
 * Not installed.
 */
#ifndef FLAKE_AMD_ROWS_PLAN_H
#define FLAKE_AMD_ROWS_PLAN_H

#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include "flakehip.h"             /* fhip_row_piece: a plain struct */

typedef struct fa_rows_counts {
    int nwhole, nwhole_pieces;    /* whole blocks; rows that have any */
    int nshort;                   /* rows with a short block */
} fa_rows_counts;

/* What fa_rows_plan will write, so that the caller can size its arrays.  Returns 0, or -1 where B < 1, a length is
 * negative or does not fit a piece's int32 count, or the whole blocks are more than an int holds. */
static inline int fa_rows_count(int nrows, const long long *len_of_row, int B, fa_rows_counts *n)
{
    long long nw = 0;
    n->nwhole = n->nwhole_pieces = n->nshort = 0;
    if (B < 1 || nrows < 0) return -1;
    for (int r = 0; r < nrows; r++) {
        const long long len = len_of_row[r];
        if (len < 0 || len > INT32_MAX) return -1;
        nw += len / B;
        if (nw > INT_MAX) return -1;
        if (len >= B) n->nwhole_pieces++;
        if (len % B) n->nshort++;
    }
    n->nwhole = (int)nw;
    return 0;
}

/* The tables.  The arrays are the caller's, exactly as large as fa_rows_count said: whole_stream [nwhole],
 * whole_pieces [nwhole_pieces], short_size / short_stream / short_pieces [nshort] each; row_first_whole [nrows + 1]
 * receives the index of every row's first whole block (the last entry: nwhole) and short_row [nshort] the row each
 * short block came from. */
static inline void fa_rows_plan(int nrows, const long long *len_of_row, const int *stream_of_row, int B,
                                int32_t *whole_stream, fhip_row_piece *whole_pieces, int32_t *short_size,
                                int32_t *short_stream, fhip_row_piece *short_pieces, int32_t *row_first_whole,
                                int32_t *short_row)
{
    int nb = 0, np = 0, ns = 0;
    long long sat = 0;                    /* where the next short block begins in its destination */
    for (int r = 0; r < nrows; r++) {
        const long long len = len_of_row[r];
        const int blocks = (int)(len / B), tail = (int)(len % B);
        row_first_whole[r] = nb;
        if (blocks > 0) {
            fhip_row_piece *q = &whole_pieces[np++];
            q->row = r; q->count = (int32_t)((long long)blocks * B); q->col = 0; q->dst = (long long)nb * B;
            for (int b = 0; b < blocks; b++) whole_stream[nb++] = stream_of_row[r];
        }
        if (tail > 0) {
            fhip_row_piece *q = &short_pieces[ns];
            q->row = r; q->count = tail; q->col = (long long)blocks * B; q->dst = sat;
            short_size[ns] = tail; short_stream[ns] = stream_of_row[r]; short_row[ns] = r;
            sat += tail;
            ns++;
        }
    }
    row_first_whole[nrows] = nb;
}

/* The part [lo, hi) of a table's destination as a table of its own, re-based to 0: what one chunk of an encode call
 * converts (fa_rc_slice for row pieces).  *cur (0 before the first slice) remembers where the walk stands, for slices
 * taken in ascending order.  out has room for n pieces.  Returns the pieces written. */
static inline int fa_rows_slice(const fhip_row_piece *tab, int n, int *cur, long long lo, long long hi, fhip_row_piece *out)
{
    int i = *cur, m = 0;
    while (i < n && tab[i].dst + tab[i].count <= lo) i++;
    *cur = i;
    for (; i < n && tab[i].dst < hi; i++) {
        const long long a = tab[i].dst > lo ? tab[i].dst : lo;
        const long long e = tab[i].dst + tab[i].count < hi ? tab[i].dst + tab[i].count : hi;
        if (e <= a) continue;
        out[m].row = tab[i].row;
        out[m].count = (int32_t)(e - a);
        out[m].col = tab[i].col + (a - tab[i].dst);
        out[m].dst = a - lo;
        m++;
    }
    return m;
}

#endif /* FLAKE_AMD_ROWS_PLAN_H */
