/*
 * held_plan.h -- the window planner (decode_window_plan.h) over HELD streams: streams whose bytes stay in a store on the
 * device and of which the host keeps a table -- every frame's size and what its header says, as k_frame_heads left it
 * (16 bytes a frame).  The accessor here answers "the header of frame k of window w's run" out of that table, so the
 * selection and the batch rule probe the same frames in the same order as they do over the bytes and a broken header
 * fails a window exactly where it does there.  Plain C on plain tables, tested and run under the sanitizers on the CPU
 * (tests/test_held_plan_cpu.py).
 * Not installed.
 */
#ifndef FLAKE_AMD_HELD_PLAN_H
#define FLAKE_AMD_HELD_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "decode_window_plan.h"

/* A frame's header as a record: fhip_frame_head's layout (flake_decode_set.c holds the two against each other). */
typedef struct fa_held_head {
    uint64_t number;
    int32_t n;
    int32_t flags;                /* bit 0: ok, bit 1: variable block size, bits 8..15: the header's length */
} fa_held_head;

/* The record of a header the predicate took (ok) or did not: what k_frame_heads writes. */
static inline fa_held_head fa_held_head_of(int ok, const flac_header *h)
{
    fa_held_head r = {0, 0, 0};
    if (ok) {
        r.number = h->number;
        r.n = h->n;
        r.flags = 1 | (h->vbs ? 2 : 0) | ((h->len & 0xFF) << 8);
    }
    return r;
}

/* One held stream: frames frame0 .. frame0 + frames of the set's size and head tables, whose offsets are entries
 * off0 .. off0 + frames + 1 of its offset table (a stream owns one more offset than frames: its end). */
typedef struct fa_held_stream {
    long long frame0, off0;
    int frames;
    unsigned fixed_block_size;
    long long samples;            /* the block sizes of its good headers added up */
} fa_held_stream;

/* The accessor: window w's run begins at record first[w] of heads. */
typedef struct fa_held_table {
    const fa_held_head *heads;
    const long long *first;
} fa_held_table;

static inline int fa_held_get(const void *ctx, int w, int k, flac_header *h)
{
    const fa_held_table *t = (const fa_held_table *)ctx;
    const fa_held_head *r = &t->heads[t->first[w] + k];
    if (!(r->flags & 1)) return 0;
    h->n = r->n;
    h->vbs = (r->flags >> 1) & 1;
    h->len = (r->flags >> 8) & 0xFF;
    h->number = r->number;
    return 1;
}

#endif
