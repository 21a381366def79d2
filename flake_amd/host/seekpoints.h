/*
 * seekpoints.h -- recording seek points while a stream is written: the recorder the encode paths feed block by block
 * (flake_host.c, flake_set.c), and the body of flake_amd_seekpoints_of_frames, the same rule over the frames of a
 * finished stream (include/flake_amd.h says what they answer).  Plain C on plain tables, in a header of its own so that
 * a stand-alone program runs it under the sanitizers on the CPU (tests/test_seekpoints_cpu.py).  Not installed.
 *
 * The rule.  The targets are k * spacing, k = 0, 1, 2, ...  A block whose samples are [first, first + samples) gets a
 * point exactly when at least one target lies in that range, and at most one: sample = first, offset = the stream's
 * bytes before the block, frame_samples = the samples of the block's first frame.  The first block always gets one.
 */
#ifndef FLAKE_AMD_SEEKPOINTS_H
#define FLAKE_AMD_SEEKPOINTS_H

#include <stddef.h>
#include <stdlib.h>

#include "flake_amd.h"
#include "../csrc/flac_header.h"

typedef struct fa_seekrec {
    unsigned long long spacing;           /* 0: recording is off */
    unsigned long long next;              /* the smallest target at or behind `samples` */
    unsigned long long samples, bytes;    /* committed to the stream so far */
    FlakeAmdSeekPoint *points;
    int n, cap;
} fa_seekrec;

/* What a rollback needs: both counters, the next target and the point count (points are only ever appended). */
typedef struct fa_seekrec_mark { unsigned long long next, samples, bytes; int n; } fa_seekrec_mark;

static inline void fa_seekrec_init(fa_seekrec *r, unsigned long long spacing)
{
    r->spacing = spacing;
    r->next = r->samples = r->bytes = 0;
    r->n = 0;
}

static inline void fa_seekrec_free(fa_seekrec *r)
{
    free(r->points);
    r->points = NULL;
    r->n = r->cap = 0;
}

static inline fa_seekrec_mark fa_seekrec_save(const fa_seekrec *r)
{
    const fa_seekrec_mark m = {r->next, r->samples, r->bytes, r->n};
    return m;
}

static inline void fa_seekrec_restore(fa_seekrec *r, const fa_seekrec_mark *m)
{
    r->next = m->next; r->samples = m->samples; r->bytes = m->bytes; r->n = m->n;
}

/* The smallest multiple of spacing at or above end (end >= 1); all ones where 64 bits cannot hold it: no sample
 * count reaches that, so nothing is recorded from there on. */
static inline unsigned long long fa_seek_target_from(unsigned long long end, unsigned long long spacing)
{
    const unsigned long long k = (end - 1) / spacing + 1;
    return k > 0xFFFFFFFFFFFFFFFFull / spacing ? 0xFFFFFFFFFFFFFFFFull : k * spacing;
}

/* One committed block: its samples per channel, its bytes (all its frames'), the samples of its first frame.
 * 0, or -1 when the point array could not grow (nothing changed). */
static inline int fa_seekrec_block(fa_seekrec *r, unsigned long long samples, unsigned long long bytes,
                                   unsigned first_frame_samples)
{
    if (!r->spacing) return 0;
    if (samples && r->next - r->samples < samples) {              /* a target in [samples so far, + samples) */
        if (r->n == r->cap) {
            const int cap = r->cap ? (r->cap > 0x3FFFFFFF ? 0x7FFFFFFF : r->cap * 2) : 64;
            FlakeAmdSeekPoint *p = cap > r->cap ? (FlakeAmdSeekPoint *)realloc(r->points, sizeof *p * (size_t)cap) : NULL;
            if (!p) return -1;
            r->points = p;
            r->cap = cap;
        }
        r->points[r->n].sample = r->samples;
        r->points[r->n].offset = r->bytes;
        r->points[r->n].frame_samples = first_frame_samples;
        r->n++;
        r->next = fa_seek_target_from(r->samples + samples, r->spacing);
    }
    r->samples += samples;
    r->bytes += bytes;
    return 0;
}

/* The same block with its first frame's samples read from that frame's own header, at d[0 .. bytes): -1 when no
 * header of the format stands there (nothing changed), or as above. */
static inline int fa_seekrec_block_at(fa_seekrec *r, const flac_format *f, const unsigned char *d,
                                      unsigned long long samples, unsigned long long bytes)
{
    if (!r->spacing) return 0;
    flac_header h;
    if (!flac_header_ok(f, d, (long long)bytes, &h)) return -1;
    return fa_seekrec_block(r, samples, bytes, (unsigned)h.n);
}

/* The first min(n, cap) points into p; returns n. */
static inline long long fa_seekrec_get(const fa_seekrec *r, FlakeAmdSeekPoint *p, int cap)
{
    for (int i = 0; i < r->n && i < cap; i++) p[i] = r->points[i];
    return r->n;
}

/* flake_amd_seekpoints_of_frames: the rule with each frame as a block, every frame's samples from its header. */
static inline long long fa_seekpoints_of_frames(const FlakeAmdStreaminfo *si, const unsigned char *stream, size_t bytes,
                                                const int *frame_sizes, int nframes, unsigned long long spacing,
                                                FlakeAmdSeekPoint *points, int cap)
{
    if (!si || nframes < 0 || cap < 0 || spacing == 0 || (cap > 0 && !points) || (nframes > 0 && (!stream || !frame_sizes)))
        return -1;
    const flac_format f = {(int)si->channels, (int)si->bits_per_sample, (int)si->sample_rate,
                           si->max_block_size > 65535u ? 0 : (int)si->max_block_size};
    unsigned long long samples = 0, next = 0;
    size_t at = 0;
    long long n = 0;
    for (int i = 0; i < nframes; i++) {
        flac_header h;
        if (frame_sizes[i] < 1 || (size_t)frame_sizes[i] > bytes - at) return -1;
        if (!flac_header_ok(&f, stream + at, (long long)frame_sizes[i], &h)) return -1;
        if (next - samples < (unsigned long long)h.n) {
            if (n < cap) {
                points[n].sample = samples;
                points[n].offset = at;
                points[n].frame_samples = (unsigned)h.n;
            }
            n++;
            next = fa_seek_target_from(samples + (unsigned long long)h.n, spacing);
        }
        samples += (unsigned long long)h.n;
        at += (size_t)frame_sizes[i];
    }
    return n;
}

#endif
