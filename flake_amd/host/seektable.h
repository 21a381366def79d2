/*
 * seektable.h -- reading a SEEKTABLE block's points and looking a sample up in them: the bodies of
 * flake_amd_read_seektable and flake_amd_seek_lookup (include/flake_amd.h says what they answer).  Plain C on plain
 * tables, in a header of its own so that a stand-alone program runs them under the sanitizers on the CPU
 * (tests/test_seektable_cpu.py).  Not installed.
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
