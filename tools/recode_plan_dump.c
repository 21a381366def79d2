/*
 * recode_plan_dump.c -- runs the recode set's planner (flake_amd/host/recode_plan.h) on a case read from standard input
 * and prints its tables.  For tests/test_recode_plan_cpu.py, which builds it plain and with the sanitizers; every array
 * is allocated exactly as large as the planner's header promises.
 *
 * Input, whitespace-separated integers:
 *   nstreams block nsegs block_cap tails_max nslices
 *   nstreams x (carry_off carry_len failed)
 *   nsegs    x (stream start samples ok)
 *   nslices  x (lo hi)                     parts of the block table's destination, ascending
 * Output:
 *   "E -1" when the blocks exceed block_cap, then the streams as they were ("S off len failed" each); else
 *   "N nblocks nblock_pieces ncarry_pieces carry_total", "P buf count src dst" per block piece, "B streams..." ,
 *   "C buf count src dst" per carry piece, "S off len failed" per stream, per slice "L count" and its "Q" pieces, and
 *   the tails in batches of tails_max: "T count pieces next", "Z size stream" each, "Y buf count src dst" each.
 */
#include <stdio.h>
#include <stdlib.h>

#include "recode_plan.h"

static long long rd(void)
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

static void piece(const char *tag, const fhip_gather_piece *q)
{
    printf("%s %d %d %lld %lld\n", tag, q->src_buf, q->count, (long long)q->src, (long long)q->dst);
}

int main(void)
{
    const int nstreams = (int)rd(), block = (int)rd(), nsegs = (int)rd(), block_cap = (int)rd();
    const int tails_max = (int)rd(), nslices = (int)rd();
    const size_t ns = (size_t)nstreams, ng = (size_t)nsegs;
    fa_rc_stream *st = (fa_rc_stream *)malloc(ns * sizeof *st);
    int32_t *seg_stream = (int32_t *)malloc(ng * sizeof(int32_t));
    int64_t *seg_start = (int64_t *)malloc(ng * sizeof(int64_t)), *seg_samples = (int64_t *)malloc(ng * sizeof(int64_t));
    unsigned char *seg_ok = (unsigned char *)malloc(ng);
    for (int s = 0; s < nstreams; s++) { st[s].carry_off = rd(); st[s].carry_len = (int)rd(); st[s].failed = (int)rd(); }
    for (int k = 0; k < nsegs; k++) {
        seg_stream[k] = (int32_t)rd(); seg_start[k] = rd(); seg_samples[k] = rd(); seg_ok[k] = (unsigned char)rd();
    }
    fa_rc_plan p;
    p.block_pieces = (fhip_gather_piece *)malloc((ns + ng) * sizeof(fhip_gather_piece));
    p.carry_pieces = (fhip_gather_piece *)malloc((ns + ng) * sizeof(fhip_gather_piece));
    p.block_stream = (int32_t *)malloc((size_t)block_cap * sizeof(int32_t));
    p.first = (int32_t *)malloc((ns + 1) * sizeof(int32_t));
    p.order = (int32_t *)malloc(ng * sizeof(int32_t));
    p.avail = (long long *)malloc(ns * sizeof(long long));
    const int nb = fa_rc_plan_batch(nstreams, st, block, nsegs, seg_stream, seg_start, seg_samples, seg_ok, block_cap, &p);
    if (nb < 0) {
        printf("E %d\n", nb);
        for (int s = 0; s < nstreams; s++) printf("S %lld %d %d\n", st[s].carry_off, st[s].carry_len, st[s].failed);
    } else {
        printf("N %d %d %d %lld\n", p.nblocks, p.nblock_pieces, p.ncarry_pieces, p.carry_total);
        for (int i = 0; i < p.nblock_pieces; i++) piece("P", &p.block_pieces[i]);
        printf("B");
        for (int b = 0; b < p.nblocks; b++) printf(" %d", p.block_stream[b]);
        printf("\n");
        for (int i = 0; i < p.ncarry_pieces; i++) piece("C", &p.carry_pieces[i]);
        for (int s = 0; s < nstreams; s++) printf("S %lld %d %d\n", st[s].carry_off, st[s].carry_len, st[s].failed);
        fhip_gather_piece *part = (fhip_gather_piece *)malloc((size_t)p.nblock_pieces * sizeof(fhip_gather_piece));
        int cur = 0;
        for (int i = 0; i < nslices; i++) {
            const long long lo = rd(), hi = rd();
            const int m = fa_rc_slice(p.block_pieces, p.nblock_pieces, &cur, lo, hi, part);
            printf("L %d\n", m);
            for (int j = 0; j < m; j++) piece("Q", &part[j]);
        }
        free(part);
        if (tails_max > 0) {
            fhip_gather_piece *tp = (fhip_gather_piece *)malloc((size_t)tails_max * sizeof(fhip_gather_piece));
            int32_t *sizes = (int32_t *)malloc((size_t)tails_max * sizeof(int32_t));
            int32_t *streams = (int32_t *)malloc((size_t)tails_max * sizeof(int32_t));
            int from = 0;
            while (from < nstreams) {
                int np = 0, next = from;
                const int n = fa_rc_plan_tails(nstreams, st, from, tails_max, tp, &np, sizes, streams, &next);
                printf("T %d %d %d\n", n, np, next);
                for (int j = 0; j < n; j++) printf("Z %d %d\n", sizes[j], streams[j]);
                for (int j = 0; j < np; j++) piece("Y", &tp[j]);
                from = next;
            }
            free(tp); free(sizes); free(streams);
        }
    }
    free(p.block_pieces); free(p.carry_pieces); free(p.block_stream); free(p.first); free(p.order); free(p.avail);
    free(st); free(seg_stream); free(seg_start); free(seg_samples); free(seg_ok);
    return 0;
}
