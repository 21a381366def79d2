/*
 * span_rows_plan.h -- the row bookkeeping of flake_amd_decode_set_span_rows and _held_span_rows (flake_decode_set.c): how
 * many rows of row_len samples, hop apart, a span of count samples has, where every span's rows lie in the call's batch,
 * what K13 (fhip_decode_frames_windows_spans) is told of a batch's segments, and what each row holds at the end.  Plain C
 * on plain tables: no call into the HIP layer, so that it is tested and run under the sanitizers on the CPU
 * (tests/test_span_rows_plan_cpu.py).  The sibling of decode_window_place.h, whose answers it reads.  Not installed.
 *
 * THE ROWS OF A SPAN.  Row j holds the span's samples [j * hop, j * hop + row_len).  A span of count samples has the rows
 * j with j * hop < count whose predecessor has not already reached the span's end:
 *   R = 0 for count == 0, else min(ceil(count / hop), 1 + ceil(max(count - row_len, 0) / hop)).
 * Every row holds at least one asked sample; for hop <= row_len the rows cover [0, count); for hop > row_len the samples
 * between two rows are skipped.  The spans' rows lie span after span.
 */
#ifndef FLAKE_AMD_SPAN_ROWS_PLAN_H
#define FLAKE_AMD_SPAN_ROWS_PLAN_H

#include <stdint.h>

#define FA_SR_MAX_ROWS 0x7FFFFFFFll
#define FA_SR_MAX_HOP 0x7FFFFFFFll

/* R.  -1 for count < 0, row_len < 1 or hop outside 1 .. 2^31 - 1. */
static inline long long fa_sr_count(long long count, long long row_len, long long hop)
{
    if (count < 0 || row_len < 1 || hop < 1 || hop > FA_SR_MAX_HOP) return -1;
    if (count == 0) return 0;
    const long long by_start = (count - 1) / hop + 1;
    const long long over = count > row_len ? count - row_len : 0;
    const long long by_end = 1 + (over ? (over - 1) / hop + 1 : 0);
    return by_start < by_end ? by_start : by_end;
}

/* span_first_row [nspans + 1]: every span's first row, and the call's rows at the end.  Returns them, or -1 for what
 * fa_sr_count refuses of any span and for more rows than rows_cap or than 2^31 - 1 (the table is unspecified then). */
static inline long long fa_sr_first_rows(int nspans, const long long *count, long long row_len, long long hop,
                                         long long rows_cap, int32_t *span_first_row)
{
    long long at = 0;
    const long long most = rows_cap < FA_SR_MAX_ROWS ? rows_cap : FA_SR_MAX_ROWS;
    if (nspans < 0 || rows_cap < 0) return -1;
    for (int s = 0; s < nspans; s++) {
        const long long r = fa_sr_count(count[s], row_len, hop);
        span_first_row[s] = (int32_t)at;
        if (r < 0 || r > most - at) return -1;
        at += r;
    }
    span_first_row[nspans] = (int32_t)at;
    return at;
}

/* What row j of a span that delivered `delivered` samples holds: clamp(delivered - j * hop, 0, row_len). */
static inline long long fa_sr_row_samples(long long delivered, long long j, long long row_len, long long hop)
{
    const long long left = delivered - j * hop;       /* (j < 2^31, hop < 2^31) */
    return left < 0 ? 0 : (left > row_len ? row_len : left);
}

/* A batch's segments as K13 takes them.  seg_row [nsegs] comes in as decode_window_place.h's fa_wp_batch leaves it for
 * the rows sink -- the segment's span, -1 for one that has failed already -- and leaves as the span's first row (-1
 * likewise); seg_nrows [nsegs] receives the span's rows.  (What fa_wp_batch leaves as the column -- what the span has
 * delivered so far -- is the segment's span position as it is.) */
static inline void fa_sr_batch(int nsegs, const int32_t *span_first_row, int32_t *seg_row, int32_t *seg_nrows)
{
    for (int k = 0; k < nsegs; k++) {
        const int s = seg_row[k];
        seg_nrows[k] = s < 0 ? 0 : span_first_row[s + 1] - span_first_row[s];
        seg_row[k] = s < 0 ? -1 : span_first_row[s];
    }
}

/* After the last batch: row_samples [span_first_row[nspans]] from what every span delivered (span_samples: -1 for a
 * failed one, whose rows all get -1). */
static inline void fa_sr_lengths(int nspans, const int32_t *span_first_row, const long long *span_samples, long long row_len,
                                 long long hop, long long *row_samples)
{
    for (int s = 0; s < nspans; s++)
        for (int32_t r = span_first_row[s]; r < span_first_row[s + 1]; r++)
            row_samples[r] = span_samples[s] < 0 ? -1 : fa_sr_row_samples(span_samples[s], r - span_first_row[s], row_len, hop);
}

#endif /* FLAKE_AMD_SPAN_ROWS_PLAN_H */
