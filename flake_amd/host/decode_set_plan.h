/*
 * decode_set_plan.h -- the batch planner of a decode set (flake_decode_set.c): which frames of which run of a call go
 * into which device batch, as the segment tables fhip_decode_frames_segments takes, the numbering each segment is held
 * to, and K6's CSR (stream -> its segments of the batch, in batch order).  Plain C on plain tables: no call into the
 * HIP layer, so that it is tested and run under the sanitizers on the CPU (tests/test_decode_set_plan_cpu.py).
 *
 * A call is nruns runs; run r is frames_of_run[r] consecutive frames of stream stream_of_run[r], all frames back to back.
 * A batch is the next frames of the call, at most max_batch of them, cut at a frame boundary wherever that falls -- inside
 * a run too; the part of a run inside a batch is one SEGMENT.  Empty runs make no segment.  A stream that has failed
 * (during this call: fa_ds_check refuses a call that names one) still gets its segments, unnumbered: its frames lie
 * between the others' and the device takes a batch's frames back to back; the set ignores what comes of them.
 * Not installed.
 */
#ifndef FLAKE_AMD_DECODE_SET_PLAN_H
#define FLAKE_AMD_DECODE_SET_PLAN_H

#include <stddef.h>
#include <stdint.h>

/* What the planner reads of a stream.  next_number is the number its next frame must carry (started streams). */
typedef struct fa_ds_stream {
    int started, variable, failed;
    long long next_number;
    int block, ended;             /* fixed blocks (fa_ds_fixed_sizes): the size every frame but the last has, 0 while no
                                     frame was committed; ended: a shorter frame was committed, none may follow */
} fa_ds_stream;

/* The size rule of a fixed-block stream ACROSS segments.  Inside a segment the device holds "every frame but the last
 * has one size, the last may be shorter"; a segment's first frame has no predecessor there, so a short frame in the
 * middle of a stream would pass wherever a batch or a run happens to be cut behind it.  The set calls this for every
 * good segment it commits, with the sizes of the segment's first and last frames (nframes >= 1; all but the last equal
 * the first, last_n <= first_n): 0 and *t moved on, or -1 when the segment follows a short frame, or does not have the
 * stream's size (one frame that is shorter may: it is then the stream's last). */
static inline int fa_ds_fixed_sizes(fa_ds_stream *t, int nframes, int first_n, int last_n)
{
    if (t->ended) return -1;
    if (!t->block) t->block = first_n;
    else if (first_n != t->block && !(nframes == 1 && first_n < t->block)) return -1;
    if (last_n < t->block) t->ended = 1;
    return 0;
}

/* Where the next batch begins: run `run`, `taken` of whose frames are planned already; `frame` and `byte` are that
 * frame's index in the call and its offset in the call's bytes.  All zero before the first batch. */
typedef struct fa_ds_cursor {
    int run, taken;
    long long frame;
    size_t byte;
} fa_ds_cursor;

/* One batch.  The arrays are the caller's: seg_first [max_batch + 1], md5_first [nstreams + 1], last_seg and planned
 * [nstreams] (scratch), every other one [max_batch]. */
typedef struct fa_ds_batch {
    long long frame0;         /* the batch's first frame in the call */
    int nframes, nsegs;
    size_t byte0, nbytes;
    int32_t *seg_first;       /* CSR over the batch's frames */
    int64_t *seg_number;      /* the number the segment's first frame must carry; -1: not held by the device */
    int32_t *seg_variable;    /* the stream's blocking strategy */
    int32_t *seg_stream, *seg_run;
    int32_t *seg_frame0;      /* the segment's first frame, counted from its run's first */
    int32_t *seg_prev;        /* the stream's previous segment in this batch, -1: none.  A variable-block-size stream's
                                 later segment cannot be numbered before the earlier one's samples are known: its
                                 seg_number is -1 and the set checks the number after the batch.  (Fixed blocks: the
                                 number is the stream's plus the frames planned before.) */
    int32_t *md5_first, *md5_range;
    int32_t *last_seg;
    long long *planned;
} fa_ds_batch;

enum { FA_DS_OK = 0, FA_DS_BAD_STREAM = -1, FA_DS_BAD_COUNT = -2, FA_DS_BAD_SIZE = -3, FA_DS_FAILED_STREAM = -4,
       FA_DS_NULL = -5 };

/* The call's arguments, before anything is changed.  *total_frames (optional) = the call's frames. */
static inline int fa_ds_check(int nstreams, const fa_ds_stream *st, int nruns, const int *stream_of_run,
                              const int *frames_of_run, const int *frame_sizes, size_t bytes, long long *total_frames)
{
    if (nruns < 0 || nstreams < 1) return FA_DS_BAD_COUNT;
    if (!st || (nruns && (!stream_of_run || !frames_of_run))) return FA_DS_NULL;
    long long nf = 0;
    for (int r = 0; r < nruns; r++) {
        if (stream_of_run[r] < 0 || stream_of_run[r] >= nstreams) return FA_DS_BAD_STREAM;
        if (frames_of_run[r] < 0) return FA_DS_BAD_COUNT;
        if (st[stream_of_run[r]].failed) return FA_DS_FAILED_STREAM;
        nf += frames_of_run[r];
    }
    if (nf && !frame_sizes) return FA_DS_NULL;
    size_t at = 0;
    for (long long f = 0; f < nf; f++) {
        if (frame_sizes[f] < 1 || (size_t)frame_sizes[f] > bytes - at) return FA_DS_BAD_SIZE;
        at += (size_t)frame_sizes[f];
    }
    if (total_frames) *total_frames = nf;
    return FA_DS_OK;
}

/* K6's CSR: stream s absorbs segments md5_range[md5_first[s] .. md5_first[s + 1]), its segments in batch order (a
 * counting sort; fhip_decode_frames_segments builds the same from seg_stream). */
static inline void fa_ds_md5_csr(int nsegs, const int32_t *seg_stream, int nstreams, int32_t *md5_first, int32_t *md5_range)
{
    for (int s = 0; s <= nstreams; s++) md5_first[s] = 0;
    for (int i = 0; i < nsegs; i++) md5_first[seg_stream[i] + 1]++;
    for (int s = 0; s < nstreams; s++) md5_first[s + 1] += md5_first[s];
    for (int i = 0; i < nsegs; i++) md5_range[md5_first[seg_stream[i]]++] = i;      /* first[s] is now first[s + 1] ... */
    for (int s = nstreams; s > 0; s--) md5_first[s] = md5_first[s - 1];             /* ... and is moved back */
    md5_first[0] = 0;
}

/* The next batch of a checked call: fills *b from *cur and moves *cur behind it.  Returns the batch's frames; 0 when the
 * call is used up (nothing of *b is valid then). */
static inline int fa_ds_plan(fa_ds_cursor *cur, int nruns, const int *stream_of_run, const int *frames_of_run,
                             const int *frame_sizes, int nstreams, const fa_ds_stream *st, int max_batch, fa_ds_batch *b)
{
    for (int s = 0; s < nstreams; s++) { b->last_seg[s] = -1; b->planned[s] = 0; }
    b->frame0 = cur->frame;
    b->byte0 = cur->byte;
    b->nframes = b->nsegs = 0;
    b->nbytes = 0;
    b->seg_first[0] = 0;
    while (cur->run < nruns && b->nframes < max_batch) {
        const int r = cur->run, left = frames_of_run[r] - cur->taken;
        if (left <= 0) { cur->run++; cur->taken = 0; continue; }        /* an empty run, or one used up */
        const int room = max_batch - b->nframes, take = left < room ? left : room;
        const int s = stream_of_run[r], k = b->nsegs++;
        const fa_ds_stream *t = &st[s];
        b->seg_stream[k] = s;
        b->seg_run[k] = r;
        b->seg_frame0[k] = cur->taken;
        b->seg_prev[k] = b->last_seg[s];
        b->seg_variable[k] = t->variable != 0;       /* (a stream not started: the bit its first frame shows) */
        if (!t->started || t->failed) b->seg_number[k] = -1;
        else if (!t->variable) b->seg_number[k] = t->next_number + b->planned[s];
        else b->seg_number[k] = b->last_seg[s] < 0 ? t->next_number : -1;
        b->last_seg[s] = k;
        b->planned[s] += take;
        for (int f = 0; f < take; f++) b->nbytes += (size_t)frame_sizes[cur->frame + f];
        b->nframes += take;
        b->seg_first[k + 1] = b->nframes;
        cur->frame += take;
        cur->taken += take;
    }
    cur->byte += b->nbytes;
    if (b->nframes) fa_ds_md5_csr(b->nsegs, b->seg_stream, nstreams, b->md5_first, b->md5_range);
    return b->nframes;
}

#endif
