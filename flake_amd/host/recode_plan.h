/*
 * recode_plan.h -- the planner of a recode set (flake_recode_set.c): how the samples one decode batch left on the device,
 * and what each stream carried over from the batches before, become the encoder's blocks -- as the piece tables K9
 * (fhip_gather_spans_dev, fhip_frames_packed_gather) takes.  Plain C on plain tables: no call into the HIP layer, so that
 * it is tested and run under the sanitizers on the CPU (tests/test_recode_plan_cpu.py).  The sibling of decode_set_plan.h.
 *
 * Two sources: buffer 0 is the CARRY buffer, every stream's samples that did not fill a block yet, dense and in stream
 * order (stream s: carry_len samples at carry_off); buffer 1 is the DECODED buffer of the batch, segment k being
 * seg_samples[k] samples at seg_start[k].  A step writes two tables:
 *   block pieces   the whole blocks of the batch, stream by stream in ascending stream order, each stream's samples in
 *                  order: its carry first, then its good segments in batch order.  They tile [0, nblocks * block).
 *   carry pieces   the NEW carry buffer, again dense and in stream order: what is left of every stream.  A stream that
 *                  got no block keeps its old carry in front of its new samples; a stream without a segment in the batch
 *                  is copied as it is.  They tile [0, sum of the new carries).
 * The carries are DOUBLE-BUFFERED: the carry pieces read the old carry buffer and the decoded buffer and write the other
 * carry buffer, so neither gather reads what the other (or itself) writes, in whatever order they run.
 *
 * A segment that is not ok fails its stream for good: the stream's good segments before it in the batch still make their
 * whole blocks, nothing behind it is taken, and the stream's carry is dropped.  A stream that comes in failed gives and
 * keeps nothing.
 * Not installed.
 */
#ifndef FLAKE_AMD_RECODE_PLAN_H
#define FLAKE_AMD_RECODE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#include "flakehip.h"             /* fhip_gather_piece: a plain struct */

enum { FA_RC_CARRY = 0, FA_RC_DECODED = 1 };       /* src_buf of a piece */

typedef struct fa_rc_stream {
    long long carry_off;          /* where its carry begins in the carry buffer (samples per channel) */
    int carry_len;                /* 0 .. block - 1 */
    int failed;
} fa_rc_stream;

/* One step's tables.  The arrays are the caller's: block_pieces and carry_pieces [nstreams + nsegs] each, block_stream
 * [block_cap], first [nstreams + 1], order [nsegs], avail [nstreams] (the last three are scratch). */
typedef struct fa_rc_plan {
    int nblocks, nblock_pieces, ncarry_pieces;
    long long carry_total;        /* samples per channel in the new carry buffer */
    fhip_gather_piece *block_pieces;
    int32_t *block_stream;
    fhip_gather_piece *carry_pieces;
    int32_t *first, *order;
    long long *avail;
} fa_rc_plan;

/* Append count samples of (buf, src) at destination *at; a piece that continues the one before it is merged into it. */
static inline void fa_rc_put(fhip_gather_piece *tab, int *n, long long *at, int buf, long long src, long long count)
{
    if (count <= 0) return;
    if (*n > 0) {
        fhip_gather_piece *q = &tab[*n - 1];
        if (q->src_buf == buf && q->src + q->count == src && (long long)q->count + count <= 0x7fffffff) {
            q->count += (int32_t)count;
            *at += count;
            return;
        }
    }
    fhip_gather_piece *q = &tab[(*n)++];
    q->src_buf = buf; q->count = (int32_t)count; q->src = src; q->dst = *at;
    *at += count;
}

/* One step.  seg_ok[k] != 0: segment k is good.  Returns the blocks, or -1 with NOTHING changed when they exceed
 * block_cap.  On success st[] describes the new carry buffer and names the streams that failed in this batch. */
static inline int fa_rc_plan_batch(int nstreams, fa_rc_stream *st, int block, int nsegs, const int32_t *seg_stream,
                                   const int64_t *seg_start, const int64_t *seg_samples, const unsigned char *seg_ok,
                                   int block_cap, fa_rc_plan *p)
{
    /* every stream's segments in batch order (a counting sort, as K6's CSR) */
    for (int s = 0; s <= nstreams; s++) p->first[s] = 0;
    for (int k = 0; k < nsegs; k++) p->first[seg_stream[k] + 1]++;
    for (int s = 0; s < nstreams; s++) p->first[s + 1] += p->first[s];
    for (int k = 0; k < nsegs; k++) p->order[p->first[seg_stream[k]]++] = k;
    for (int s = nstreams; s > 0; s--) p->first[s] = p->first[s - 1];
    p->first[0] = 0;
    /* what each stream has: its carry and its good segments up to the first bad one */
    long long blocks = 0;
    for (int s = 0; s < nstreams; s++) {
        long long have = st[s].failed ? 0 : st[s].carry_len;
        for (int i = p->first[s]; i < p->first[s + 1] && !st[s].failed; i++) {
            const int k = p->order[i];
            if (!seg_ok[k]) break;
            if (seg_samples[k] > 0) have += seg_samples[k];
        }
        p->avail[s] = have;
        blocks += have / block;
    }
    if (blocks > block_cap) return -1;
    int nb = 0, nbp = 0, ncp = 0;
    long long bat = 0, cat = 0;
    for (int s = 0; s < nstreams; s++) {
        fa_rc_stream *t = &st[s];
        int bad = t->failed;
        for (int i = p->first[s]; i < p->first[s + 1] && !bad; i++) bad = !seg_ok[p->order[i]];
        const long long have = p->avail[s], to_blocks = have / block * block;
        long long left = to_blocks;                   /* samples still to go to blocks; the rest goes to the carry */
        const long long new_off = cat;
        /* the carry, then the good segments: each span first fills the blocks, what is over goes to the new carry */
        for (int i = -1; i < p->first[s + 1] - p->first[s] && !t->failed; i++) {
            long long src, n;
            int buf;
            if (i < 0) { buf = FA_RC_CARRY; src = t->carry_off; n = t->carry_len; }
            else {
                const int k = p->order[p->first[s] + i];
                if (!seg_ok[k]) break;
                buf = FA_RC_DECODED; src = seg_start[k]; n = seg_samples[k] > 0 ? seg_samples[k] : 0;
            }
            const long long head = n < left ? n : left;
            fa_rc_put(p->block_pieces, &nbp, &bat, buf, src, head);
            left -= head;
            if (!bad) fa_rc_put(p->carry_pieces, &ncp, &cat, buf, src + head, n - head);
        }
        for (long long b = 0; b < to_blocks / block; b++) p->block_stream[nb++] = s;
        if (bad) t->failed = 1;
        t->carry_off = new_off;
        t->carry_len = (int)(cat - new_off);
    }
    p->nblocks = nb; p->nblock_pieces = nbp; p->ncarry_pieces = ncp;
    p->carry_total = cat;
    return nb;
}

/* The part [lo, hi) of a table's destination as a table of its own, re-based to 0: what one chunk of an encode call
 * gathers.  *cur (0 before the first slice) remembers where the walk stands, for slices taken in ascending order.
 * out has room for n pieces.  Returns the pieces written. */
static inline int fa_rc_slice(const fhip_gather_piece *tab, int n, int *cur, long long lo, long long hi,
                              fhip_gather_piece *out)
{
    int i = *cur, m = 0;
    while (i < n && tab[i].dst + tab[i].count <= lo) i++;
    *cur = i;
    for (; i < n && tab[i].dst < hi; i++) {
        const long long a = tab[i].dst > lo ? tab[i].dst : lo;
        const long long e = tab[i].dst + tab[i].count < hi ? tab[i].dst + tab[i].count : hi;
        if (e <= a) continue;
        out[m].src_buf = tab[i].src_buf;
        out[m].count = (int32_t)(e - a);
        out[m].src = tab[i].src + (a - tab[i].dst);
        out[m].dst = a - lo;
        m++;
    }
    return m;
}

/* The tails at the end: every good stream's carry from stream `from` on, at most max of them, as one ragged batch read
 * from the carry buffer.  pieces, sizes, streams: [max] each.  *next = the stream to go on from.  Returns the tails. */
static inline int fa_rc_plan_tails(int nstreams, const fa_rc_stream *st, int from, int max, fhip_gather_piece *pieces,
                                   int *npieces, int32_t *sizes, int32_t *streams, int *next)
{
    int n = 0, np = 0;
    long long at = 0;
    int s = from;
    for (; s < nstreams && n < max; s++) {
        if (st[s].failed || st[s].carry_len < 1) continue;
        sizes[n] = st[s].carry_len;
        streams[n] = s;
        n++;
        fa_rc_put(pieces, &np, &at, FA_RC_CARRY, st[s].carry_off, st[s].carry_len);
    }
    *npieces = np;
    *next = s;
    return n;
}

#endif
