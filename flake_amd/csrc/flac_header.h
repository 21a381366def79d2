/*
 * flac_header.h -- what a FLAC frame header's codes mean, and the one predicate "a header of this stream stands
 * here", for every reader of frames: the host indexer and decoder (host/flake_decode.c, host/flake_decode_set.c), K8
 * (k8_index.hip) and, for the tables and the CRC-8 step, K5's and K7's parser (flac_parse.h).  The common subset of
 * C99 and C++17: gcc compiles it for the host layer, hipcc for host and device.  No table in memory, no global state.
 */
#ifndef FLAKE_AMD_FLAC_HEADER_H
#define FLAKE_AMD_FLAC_HEADER_H

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define FLAC_HEADER_FN __host__ __device__ static inline
#else
#define FLAC_HEADER_FN static inline
#endif

/* What a header's codes are held against: STREAMINFO's values.  max_block_size 0: no limit. */
typedef struct flac_format { int channels, bps, sample_rate, max_block_size; } flac_format;

/* An accepted header: block size, blocking-strategy bit, header length in bytes (CRC-8 included), the coded frame or
 * sample number. */
typedef struct flac_header { int n, vbs, len; unsigned long long number; } flac_header;

/* Does sample-rate code 0 .. 11 stand for rate?  0 is "as STREAMINFO says"; 12 .. 14 carry the rate behind the number
 * (checked there) and 15 is invalid: all four answer 0 here. */
FLAC_HEADER_FN int flac_rate_code_ok(int code, int rate)
{
    switch (code) {
    case 0: return 1;
    case 1: return rate == 88200;
    case 2: return rate == 176400;
    case 3: return rate == 192000;
    case 4: return rate == 8000;
    case 5: return rate == 16000;
    case 6: return rate == 22050;
    case 7: return rate == 24000;
    case 8: return rate == 32000;
    case 9: return rate == 44100;
    case 10: return rate == 48000;
    case 11: return rate == 96000;
    default: return 0;
    }
}

/* The sample-size code of bps bits; -1: there is none (such a stream's headers carry code 0). */
FLAC_HEADER_FN int flac_bps_code(int bps)
{
    switch (bps) {
    case 8: return 1;
    case 12: return 2;
    case 16: return 4;
    case 20: return 5;
    case 24: return 6;
    case 32: return 7;
    default: return -1;
    }
}

/* The block size of block-size code 1 .. 5 and 8 .. 15; 0 for 6 and 7 (the size follows the number) and for 0. */
FLAC_HEADER_FN int flac_block_size_of_code(int bs_code)
{
    return bs_code == 1 ? 192 : (bs_code <= 5 ? 576 << (bs_code - 2) : (bs_code >= 8 ? 256 << (bs_code - 8) : 0));
}

/* CRC-8, polynomial x^8 + x^2 + x + 1, zero init: c moved on by byte b. */
FLAC_HEADER_FN unsigned flac_crc8_step(unsigned c, unsigned b)
{
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) : (c << 1);
    return c & 0xFFu;
}

/* 1 when the header at d[0 .. avail) is one whose codes agree with f and whose CRC-8 holds (*h is filled), else 0.
 * Never reads at or past avail.  Block sizes above 65535 are refused: STREAMINFO cannot describe them. */
FLAC_HEADER_FN int flac_header_ok(const flac_format *f, const unsigned char *d, long long avail, flac_header *h)
{
    if (avail < 6 || d[0] != 0xFF || (d[1] & 0xFE) != 0xF8) return 0;
    const int bs_code = d[2] >> 4, sr_code = d[2] & 15, ch_code = d[3] >> 4, bps_code = (d[3] >> 1) & 7;
    if (bs_code == 0 || sr_code == 15 || (d[3] & 1)) return 0;
    if (sr_code < 12 && !flac_rate_code_ok(sr_code, f->sample_rate)) return 0;
    if (ch_code > 10 || (ch_code < 8 && ch_code + 1 != f->channels) || (ch_code >= 8 && f->channels != 2)) return 0;
    if (bps_code != 0 && bps_code != flac_bps_code(f->bps)) return 0;
    /* UTF-8 style number: 1 .. 7 bytes, up to 36 bits */
    long long p = 4;
    const unsigned b0 = d[p++];
    int extra = 0;
    unsigned long long num = b0;
    if (b0 >= 0x80u) {
        int ones = 0;
        while (ones < 8 && ((b0 << ones) & 0x80u)) ones++;
        if (ones < 2 || ones > 7) return 0;
        extra = ones - 1;
        num = ones == 7 ? 0 : (b0 & (0x7Fu >> ones));
    }
    if (p + extra > avail) return 0;
    for (int i = 0; i < extra; i++) {
        const unsigned c = d[p++];
        if ((c & 0xC0u) != 0x80u) return 0;
        num = (num << 6) | (c & 0x3Fu);
    }
    int n = flac_block_size_of_code(bs_code);
    if (bs_code == 6) {
        if (p + 1 > avail) return 0;
        n = d[p] + 1;
        p += 1;
    } else if (bs_code == 7) {
        if (p + 2 > avail) return 0;
        n = (d[p] << 8 | d[p + 1]) + 1;
        p += 2;
    }
    if (n > 65535 || (f->max_block_size && n > f->max_block_size)) return 0;
    if (sr_code >= 12) {
        const int nb = sr_code == 12 ? 1 : 2;
        if (p + nb > avail) return 0;
        const long long v = nb == 1 ? d[p] : (d[p] << 8 | d[p + 1]);
        const long long rate = sr_code == 12 ? v * 1000 : (sr_code == 13 ? v : v * 10);
        if (rate != f->sample_rate) return 0;
        p += nb;
    }
    if (p + 1 > avail) return 0;
    unsigned c8 = 0;
    for (long long i = 0; i < p; i++) c8 = flac_crc8_step(c8, d[i]);
    if (c8 != d[p]) return 0;
    h->n = n;
    h->vbs = d[1] & 1;
    h->len = (int)p + 1;
    h->number = num;
    return 1;
}

#endif
