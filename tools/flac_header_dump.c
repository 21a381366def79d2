/*
 * flac_header_dump.c -- runs the frame-header predicate (flake_amd/csrc/flac_header.h) on cases read from standard
 * input and prints its verdicts.  tests/test_flac_header_cpu.py builds it as C99, as C++17 and with
 * -fsanitize=address,undefined, and holds the three outputs to each other and to a parser of its own.  Every case's
 * bytes lie in an allocation of exactly `avail` bytes, so a read at or past avail is reported.  No GPU, no HIP.
 *
 * Input (words, any white space):  "F channels bps sample_rate max_block_size"   the format of the cases that follow
 *                                  "C avail hex"                                  a case: avail bytes as 2 * avail hex
 *                                                                                 digits ("-" for none)
 * Output, a line per case:  "0" (refused) or "1 n vbs len number".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flac_header.h"

static int hex(int c) { return c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1); }

static void bad(const char *what)
{
    fprintf(stderr, "bad input: %s\n", what);
    exit(2);
}

int main(void)
{
    flac_format f = {0, 0, 0, 0};
    char word[8], digits[128];
    while (scanf("%7s", word) == 1) {
        if (!strcmp(word, "F")) {
            if (scanf("%d %d %d %d", &f.channels, &f.bps, &f.sample_rate, &f.max_block_size) != 4) bad("format");
            continue;
        }
        long long avail = -1;
        if (strcmp(word, "C") || scanf("%lld %127s", &avail, digits) != 2 || avail < 0) bad("case");
        if (strcmp(digits, "-") ? strlen(digits) != 2 * (size_t)avail : avail != 0) bad("length");
        unsigned char *d = (unsigned char *)malloc((size_t)avail);
        for (long long i = 0; i < avail; i++) {
            const int hi = hex(digits[2 * i]), lo = hex(digits[2 * i + 1]);
            if (hi < 0 || lo < 0) bad("hex digit");
            d[i] = (unsigned char)(hi << 4 | lo);
        }
        flac_header h;
        if (flac_header_ok(&f, d, avail, &h)) printf("1 %d %d %d %llu\n", h.n, h.vbs, h.len, h.number);
        else printf("0\n");
        free(d);
    }
    return 0;
}
