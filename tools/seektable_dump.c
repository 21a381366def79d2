/*
 * seektable_dump.c -- runs the SEEKTABLE reader and the lookup (flake_amd/host/seektable.h) on a block read from
 * standard input.  tests/test_seektable_cpu.py builds it with -fsanitize=address,undefined and holds its output to the
 * library's: the block and the point table are exactly as large as the input says.  No GPU, no HIP.
 *
 * Input (integers):  bytes cap nlookups   bytes x { byte }   nlookups x { sample }
 * Output:  "N <return value>", per stored point "P sample offset frame_samples", per lookup "L <index>".
 */
#include <stdio.h>
#include <stdlib.h>

#include "seektable.h"

static unsigned long long rd(void)
{
    unsigned long long v = 0;
    if (scanf("%llu", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(void)
{
    const size_t bytes = (size_t)rd();
    const int cap = (int)rd(), nl = (int)rd();
    unsigned char *block = (unsigned char *)malloc(bytes ? bytes : 1);
    FlakeAmdSeekPoint *pts = (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)(cap > 0 ? cap : 1));
    for (size_t i = 0; i < bytes; i++) block[i] = (unsigned char)rd();
    const long long n = fa_read_seektable(block, bytes, pts, cap);
    printf("N %lld\n", n);
    const int have = n < 0 ? 0 : (n < cap ? (int)n : cap);
    for (int i = 0; i < have; i++) printf("P %llu %llu %u\n", pts[i].sample, pts[i].offset, pts[i].frame_samples);
    for (int i = 0; i < nl; i++) printf("L %lld\n", fa_seek_lookup(pts, have, rd()));
    free(block);
    free(pts);
    return 0;
}
