/*
 * flake_decode.c -- the host layer's decoding side: STREAMINFO read back, frame discovery in a foreign stream
 * (on the CPU: it is a search, byte by byte, with a CRC-16 over every candidate span), and a decoder object that
 * hands batches of indexed frames to fhip_decode_frames (K7), carries the expected number from call to call and
 * hashes what it returns, so that the caller can hold it against STREAMINFO's MD5.
 *
 * flake_amd_read_streaminfo and flake_amd_index_frames make no call into the HIP layer.  flake_amd_decode_index is the
 * same discovery on the device (fhip_index_frames, K8), held to flake_amd_index_frames' answer.  What counts as a frame
 * header is csrc/flac_header.h's predicate, the source K8 compiles too.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"
#include "flakehip.h"
#include "host_internal.h"
#include "seektable.h"
#include "seekpoints.h"

/* ---- STREAMINFO ------------------------------------------------------ */

FLAKE_AMD_API int flake_amd_read_streaminfo(const unsigned char d[34], FlakeAmdStreaminfo *si)
{
    if (!d || !si) return -1;
    si->min_block_size = (unsigned)d[0] << 8 | d[1];
    si->max_block_size = (unsigned)d[2] << 8 | d[3];
    si->min_frame_size = (unsigned)d[4] << 16 | (unsigned)d[5] << 8 | d[6];
    si->max_frame_size = (unsigned)d[7] << 16 | (unsigned)d[8] << 8 | d[9];
    si->sample_rate = (unsigned)d[10] << 12 | (unsigned)d[11] << 4 | (unsigned)d[12] >> 4;
    si->channels = ((d[12] >> 1) & 7u) + 1u;
    si->bits_per_sample = (((unsigned)d[12] & 1u) << 4 | (unsigned)d[13] >> 4) + 1u;
    si->samples = (unsigned)d[14] << 24 | (unsigned)d[15] << 16 | (unsigned)d[16] << 8 | d[17];
    memcpy(si->md5sum, d + 18, 16);
    if (si->sample_rate == 0 || si->sample_rate > 655350u || si->bits_per_sample < 4) return -1;
    return d[13] & 15;          /* bits 32..35 of the sample count, which the struct's 32-bit field cannot hold */
}

/* ---- a frame header ---------------------------------------------------- */

/* flac_header_ok (csrc/flac_header.h) held against STREAMINFO: 0 when a header of this stream stands at
 * d[0 .. avail), else -1.  A max_block_size above what a header can carry limits nothing.  (Also for
 * flake_decode_set.c: host_internal.h.) */
int fa_parse_header(const FlakeAmdStreaminfo *si, const unsigned char *d, size_t avail, flac_header *h)
{
    const flac_format f = {(int)si->channels, (int)si->bits_per_sample, (int)si->sample_rate,
                           si->max_block_size > 65535u ? 0 : (int)si->max_block_size};
    return flac_header_ok(&f, d, (long long)avail, h) ? 0 : -1;
}

/* ---- SEEKTABLE ----------------------------------------------------------- */

FLAKE_AMD_API long long flake_amd_read_seektable(const unsigned char *block, size_t bytes, FlakeAmdSeekPoint *points, int cap)
{
    return fa_read_seektable(block, bytes, points, cap);
}

FLAKE_AMD_API long long flake_amd_seek_lookup(const FlakeAmdSeekPoint *points, int n, unsigned long long sample)
{
    return fa_seek_lookup(points, n, sample);
}

FLAKE_AMD_API long long flake_amd_write_seektable(const FlakeAmdSeekPoint *points, int n, int placeholders,
                                                  unsigned char *block, size_t cap)
{
    return fa_write_seektable(points, n, placeholders, block, cap);
}

FLAKE_AMD_API long long flake_amd_seekpoints_of_frames(const FlakeAmdStreaminfo *si, const unsigned char *stream, size_t bytes,
                                                       const int *frame_sizes, int nframes, unsigned long long spacing,
                                                       FlakeAmdSeekPoint *points, int cap)
{
    return fa_seekpoints_of_frames(si, stream, bytes, frame_sizes, nframes, spacing, points, cap);
}

/* ---- frame discovery --------------------------------------------------- */

FLAKE_AMD_API long long flake_amd_index_frames(const FlakeAmdStreaminfo *si, const unsigned char *s, size_t bytes,
                                               int *frame_sizes, int cap, size_t *consumed)
{
    if (consumed) *consumed = 0;
    if (!si || (!s && bytes) || !frame_sizes || cap < 0) return -1;
    unsigned short tab[256];                    /* CRC-16, polynomial 0x8005, a byte at a time */
    for (int b = 0; b < 256; b++) {
        unsigned c = (unsigned)b << 8;
        for (int k = 0; k < 8; k++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        tab[b] = (unsigned short)c;
    }
    if (bytes == 0 || cap == 0) return 0;
    flac_header cur;
    if (fa_parse_header(si, s, bytes, &cur)) return -1;         /* garbage at the start */
    const int vbs = cur.vbs;
    size_t start = 0;
    long long count = 0;
    while (count < cap) {
        /* the frame at `start` ends at the first q where the CRC-16 of [start, q - 2) is what lies at q - 2 and
         * either the stream ends or the next frame's header begins: the expected number, CRC-8 and all */
        const unsigned long long want = cur.number + (vbs ? (unsigned long long)cur.n : 1ull);
        size_t k = start, end = 0;
        unsigned crc = 0;                       /* of [start, k) */
        flac_header next;
        memset(&next, 0, sizeof next);
        for (size_t q = start + (size_t)cur.len + 2; q <= bytes; q++) {
            while (k < q - 2) crc = ((crc << 8) & 0xFFFFu) ^ tab[((crc >> 8) ^ s[k++]) & 0xFFu];
            if (crc != ((unsigned)s[q - 2] << 8 | s[q - 1])) continue;
            if (q == bytes) { end = q; break; }
            flac_header h;
            if (fa_parse_header(si, s + q, bytes - q, &h) == 0 && h.vbs == vbs && h.number == want) {
                end = q;
                next = h;
                break;
            }
        }
        if (!end) break;                        /* cut inside this frame (or no valid end): it is not consumed */
        frame_sizes[count++] = (int)(end - start);
        if (consumed) *consumed = end;
        if (end == bytes) break;
        start = end;
        cur = next;
    }
    return count;
}

/* ---- the decoder object ------------------------------------------------ */

struct FlakeAmdDecoder {
    fhip_ctx *hip;
    FlakeAmdStreaminfo si;
    int max_batch;
    int started, vbs;                     /* the blocking strategy, read from the first frame ever seen */
    long long next_number;                /* the number the next frame must carry */
    long long frames_done;                /* frames decoded so far (error texts count from the stream's first) */
    fa_md5 md5;
    fhip_verify_rec *recs;
    char err[384];
};

static char g_open_err[256];

FLAKE_AMD_API FlakeAmdDecoder *flake_amd_decode_open(const FlakeAmdStreaminfo *si)
{
    g_open_err[0] = 0;
    if (!si || si->channels < 1 || si->channels > 8 || si->bits_per_sample < 4 || si->bits_per_sample > 32 ||
        si->sample_rate < 1 || si->sample_rate > 655350u || si->max_block_size > 65535u) {
        snprintf(g_open_err, sizeof g_open_err, "STREAMINFO is out of range");
        return NULL;
    }
    FlakeAmdDecoder *d = (FlakeAmdDecoder *)calloc(1, sizeof *d);
    if (!d) return NULL;
    d->si = *si;
    const char *eb = getenv("FLAKE_AMD_BATCH"), *ed = getenv("FLAKE_AMD_DEVICE");
    d->max_batch = eb ? atoi(eb) : 1024;
    if (d->max_batch < 1) d->max_batch = 1;
    /* the handle: only channels, sample rate, bits per sample and the largest block matter to K7; the rest is a
     * valid encoder preset.  Its workspaces hold max_batch blocks of the largest size: a stream of very long blocks
     * gets fewer frames per batch (about 4M samples per channel). */
    int bs = si->max_block_size ? (int)si->max_block_size : 65535;
    if (bs < 16) bs = 16;
    if ((long long)d->max_batch * bs > (4ll << 20)) d->max_batch = (int)((4ll << 20) / bs);
    if (d->max_batch < 1) d->max_batch = 1;
    fhip_params p;
    memset(&p, 0, sizeof p);
    p.channels = (int)si->channels; p.sample_rate = (int)si->sample_rate; p.bits_per_sample = (int)si->bits_per_sample;
    p.block_size = bs; p.order_method = 1; p.stereo_method = 1; p.prediction_type = 2;
    p.min_prediction_order = 1; p.max_prediction_order = 8; p.min_partition_order = 0; p.max_partition_order = 5;
    p.lpc_precision = 15;
    const int rc = fhip_create(&d->hip, ed ? atoi(ed) : 0, &p, d->max_batch);
    d->recs = (fhip_verify_rec *)malloc(sizeof(fhip_verify_rec) * (size_t)d->max_batch);
    if (rc != FHIP_OK || !d->recs) {
        snprintf(g_open_err, sizeof g_open_err, "fhip_create: %s", fhip_strerror(rc));
        flake_amd_decode_close(d);
        return NULL;
    }
    fa_md5_init(&d->md5);
    return d;
}

FLAKE_AMD_API long long flake_amd_decode_frames(FlakeAmdDecoder *d, const unsigned char *stream, size_t bytes,
                                                const int *frame_sizes, int nframes, void *pcm, int sample_bytes,
                                                size_t pcm_cap_samples)
{
    if (!d) return -1;
    d->err[0] = 0;
    if ((!stream && bytes) || (!frame_sizes && nframes) || nframes < 0 || (!pcm && pcm_cap_samples) ||
        (sample_bytes != 2 && sample_bytes != 4)) {
        snprintf(d->err, sizeof d->err, "bad argument");
        return -1;
    }
    if (sample_bytes == 2 && d->si.bits_per_sample > 16) {
        snprintf(d->err, sizeof d->err, "2-byte samples need bits_per_sample <= 16");
        return -1;
    }
    if (fhip_set_pcm_format(d->hip, sample_bytes == 2 ? FHIP_PCM_S16 : FHIP_PCM_S32) != FHIP_OK) {
        snprintf(d->err, sizeof d->err, "%s", fhip_last_error(d->hip));
        return -1;
    }
    if (nframes && !d->started) {
        flac_header h;
        if (frame_sizes[0] < 1 || (size_t)frame_sizes[0] > bytes || fa_parse_header(&d->si, stream, (size_t)frame_sizes[0], &h)) {
            snprintf(d->err, sizeof d->err, "frame 0: not a frame header of this stream");
            return -1;
        }
        d->started = 1;
        d->vbs = h.vbs;
        d->next_number = (long long)h.number;
    }
    const size_t nch = d->si.channels;
    size_t off = 0, done = 0;
    for (int f0 = 0; f0 < nframes; f0 += d->max_batch) {
        const int cnt = nframes - f0 < d->max_batch ? nframes - f0 : d->max_batch;
        size_t cb = 0;
        for (int f = 0; f < cnt; f++) cb += frame_sizes[f0 + f] > 0 ? (size_t)frame_sizes[f0 + f] : 0;
        if (off + cb > bytes) {
            snprintf(d->err, sizeof d->err, "the frame sizes run past the stream");
            return -1;
        }
        int64_t summary[4] = {0, 0, -1, 0}, ns = 0;
        fhip_decode_in in = {stream + off, (int64_t)cb, frame_sizes + f0, cnt, d->vbs, d->next_number};
        fhip_decode_out out = {(int32_t *)((char *)pcm + done * nch * (size_t)sample_bytes),
                               (int64_t)(pcm_cap_samples - done), d->recs, summary, &ns};
        const int rc = fhip_decode_frames(d->hip, &in, &out);
        if (rc == FHIP_E_VERIFY) {
            static const char *const names[] = {"OK", "HEADER", "CRC8", "NUMBER", "SYNTAX", "SAMPLES", "PADDING", "CRC16", "LENGTH"};
            const long long bad = summary[2] >= 0 ? summary[2] : 0;
            const int st = (int)summary[3];
            snprintf(d->err, sizeof d->err, "frame %lld (frame %lld of this call): %s, subframe %d, bit %d; %lld of the batch's %lld frames failed",
                     d->frames_done + bad, (long long)f0 + bad, st >= 0 && st <= 8 ? names[st] : "?",
                     (int)d->recs[bad].subframe, (int)d->recs[bad].bit, (long long)summary[1], (long long)summary[0]);
            return -1;
        }
        if (rc != FHIP_OK) {
            snprintf(d->err, sizeof d->err, "fhip_decode_frames: %s", fhip_last_error(d->hip));
            return -1;
        }
        /* every frame was good: ns samples, numbered on from the last header's */
        const size_t vals = (size_t)ns * nch;
        if (sample_bytes == 2) fa_md5_pcm16(&d->md5, (const int16_t *)pcm + done * nch, vals, (int)d->si.bits_per_sample);
        else fa_md5_pcm(&d->md5, (const int32_t *)pcm + done * nch, vals, (int)d->si.bits_per_sample);
        d->next_number += d->vbs ? (long long)ns : (long long)cnt;
        d->frames_done += cnt;
        done += (size_t)ns;
        off += cb;
    }
    return (long long)done;
}

/* ---- frame discovery on the device ------------------------------------- */

int fa_index_ranges(struct fhip_ctx *hip, unsigned max_block_size, const unsigned char *stream, const size_t *range_first,
                    int nranges, int *frame_sizes, int cap, long long *range_frames, size_t *range_consumed, char *err,
                    size_t err_len)
{
    if (!hip || !range_first || nranges < 1 || cap < 0 || (!frame_sizes && cap) || !range_frames || !range_consumed ||
        range_first[0] != 0 || (!stream && range_first[nranges]))
        return -1;
    for (int r = 0; r < nranges; r++)
        if (range_first[r + 1] < range_first[r]) return -1;
    if (range_first[nranges] >= ((size_t)1 << 31)) {
        snprintf(err, err_len, "the device indexes less than 2 GiB per call");
        return -2;
    }
    const size_t nr = (size_t)nranges;
    /* one block: range_first and consumed as int64, then frames and variable as int32 */
    int64_t *w = (int64_t *)malloc((2 * nr + 1) * sizeof(int64_t) + 2 * nr * sizeof(int32_t));
    if (!w) { snprintf(err, err_len, "out of memory"); return -2; }
    int64_t *first = w, *cons = w + nr + 1;
    int32_t *frames = (int32_t *)(w + 2 * nr + 1), *variable = frames + nr;
    for (size_t r = 0; r <= nr; r++) first[r] = (int64_t)range_first[r];
    fhip_index_in in = {stream, first[nr], first, nranges, (int32_t)(max_block_size > 65535u ? 65535u : max_block_size), cap};   /* (no block is larger) */
    fhip_index_out out = {frame_sizes, frames, cons, variable};
    const int rc = fhip_index_frames(hip, &in, &out);
    if (rc != FHIP_OK) {
        snprintf(err, err_len, "fhip_index_frames: %s", fhip_last_error(hip));
        free(w);
        return -2;
    }
    for (size_t r = 0; r < nr; r++) {
        range_frames[r] = frames[r];
        range_consumed[r] = (size_t)cons[r];
    }
    free(w);
    return 0;
}

FLAKE_AMD_API long long flake_amd_decode_index(FlakeAmdDecoder *d, const unsigned char *stream, size_t bytes,
                                               int *frame_sizes, int cap, size_t *consumed)
{
    if (consumed) *consumed = 0;
    if (!d) return -1;
    d->err[0] = 0;
    if ((!stream && bytes) || !frame_sizes || cap < 0) return -1;      /* flake_amd_index_frames' own refusals */
    const size_t first[2] = {0, bytes};
    long long frames = 0;
    size_t cons = 0;
    const int rc = fa_index_ranges(d->hip, d->si.max_block_size, stream, first, 1, frame_sizes, cap, &frames, &cons, d->err,
                                   sizeof d->err);
    if (rc) return rc;
    if (consumed) *consumed = cons;
    return frames;
}

FLAKE_AMD_API int flake_amd_decode_md5(FlakeAmdDecoder *d, unsigned char md5[16])
{
    if (!d || !md5) return -1;
    fa_md5_final(&d->md5, md5);
    return 0;
}

FLAKE_AMD_API const char *flake_amd_decode_last_error(const FlakeAmdDecoder *d)
{
    return d ? d->err : g_open_err;
}

FLAKE_AMD_API void flake_amd_decode_close(FlakeAmdDecoder *d)
{
    if (!d) return;
    if (d->hip) { (void)fhip_sync(d->hip); fhip_destroy(d->hip); }
    free(d->recs);
    free(d);
}
