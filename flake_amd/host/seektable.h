/*
 * seektable.h -- reading a SEEKTABLE block's points, looking a sample up in them and writing such a block: the bodies
 * of flake_amd_read_seektable, flake_amd_seek_lookup and flake_amd_write_seektable (include/flake_amd.h says what they
 * answer).  Plain C on plain tables, in a header of its own so that a stand-alone program runs them under the
 * sanitizers on the CPU (tests/test_seektable_cpu.py).  Not installed.
 */
#ifndef FLAKE_AMD_SEEKTABLE_H
#define FLAKE_AMD_SEEKTABLE_H

#include <stddef.h>

#include "flake_amd.h"

static inline unsigned long long fa_be_u64(const unsigned char *d)
{
    unsigned long long v = 0;
    for (int i = 0; i < 8; i++) v = v << 8 | d[i];
    return v;
}

static inline long long fa_read_seektable(const unsigned char *block, size_t bytes, FlakeAmdSeekPoint *points, int cap)
{
    if ((!block && bytes) || cap < 0 || (cap > 0 && !points) || bytes % 18) return -1;
    long long n = 0;
    unsigned long long last = 0;
    for (size_t at = 0; at < bytes; at += 18) {
        const unsigned long long sample = fa_be_u64(block + at);
        if (sample == 0xFFFFFFFFFFFFFFFFull) continue;             /* a placeholder */
        if (n > 0 && sample <= last) return -1;
        last = sample;
        if (n < cap) {
            points[n].sample = sample;
            points[n].offset = fa_be_u64(block + at + 8);
            points[n].frame_samples = (unsigned)block[at + 16] << 8 | block[at + 17];
        }
        n++;
    }
    return n;
}

/* The inverse: n points and `placeholders` placeholder points behind them into block[0 .. cap).  Everything is checked
 * before the first byte is written. */
#define FA_SEEKTABLE_MAX_POINTS 932067      /* a metadata block's length has 24 bits: (2^24 - 1) / 18 */

static inline long long fa_write_seektable(const FlakeAmdSeekPoint *points, int n, int placeholders,
                                           unsigned char *block, size_t cap)
{
    if (n < 0 || placeholders < 0 || (n > 0 && !points)) return -1;
    const long long all = (long long)n + placeholders;
    if (all > FA_SEEKTABLE_MAX_POINTS || (all > 0 && !block) || cap < (size_t)all * 18) return -1;
    for (int i = 0; i < n; i++)
        if (points[i].sample == 0xFFFFFFFFFFFFFFFFull || (i > 0 && points[i].sample <= points[i - 1].sample) ||
            points[i].frame_samples > 0xFFFFu)
            return -1;
    for (long long i = 0; i < all; i++) {
        unsigned char *d = block + 18 * i;
        const unsigned long long sample = i < n ? points[i].sample : 0xFFFFFFFFFFFFFFFFull;
        const unsigned long long offset = i < n ? points[i].offset : 0;
        const unsigned fs = i < n ? points[i].frame_samples : 0;
        for (int k = 0; k < 8; k++) {
            d[k] = (unsigned char)(sample >> (56 - 8 * k));
            d[8 + k] = (unsigned char)(offset >> (56 - 8 * k));
        }
        d[16] = (unsigned char)(fs >> 8);
        d[17] = (unsigned char)fs;
    }
    return all * 18;
}

static inline long long fa_seek_lookup(const FlakeAmdSeekPoint *points, int n, unsigned long long sample)
{
    if (!points || n <= 0) return -1;
    long long lo = -1, hi = n - 1;                                  /* the answer lies in [lo, hi] */
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (points[mid].sample <= sample) lo = mid; else hi = mid - 1;
    }
    return lo;
}

#endif
