/*
 * flake_amd_cli.c -- minimal command-line encoder on top of the host layer:
 * the block loop of the reference CLI (flake/flake.c:495-689: read a block of
 * samples, flake_encode_frame(), write the frame, rewrite STREAMINFO at the
 * end), with the frames of many blocks encoded per GPU batch.
 *
 *   flake_amd_cli [-0..-12] [-b blocksize] [--verify] in.wav out.flac
 *   flake_amd_cli [-0..-12] --synth FRAMES [--channels C] [--bps B] [--verify] out.flac
 *   flake_amd_cli [-0..-12] [-b blocksize] --set OUTDIR [--verify] in1.wav in2.wav ...
 *   flake_amd_cli [-0..-12] --set OUTDIR [--verify] --synth-streams S --synth FRAMES [--channels C] [--bps B]
 *
 * --set encodes inputs of one format as a stream set (flake_amd_set_*): their blocks round-robin in shared GPU
 * batches, every stream's MD5 carried on the device, one OUTDIR/<name>.flac per input with its own STREAMINFO --
 * the file the single-input form writes for that input.
 *
 * --verify checks on the GPU that every frame decodes to its input (flake_amd_set_verify; for --set
 * flake_amd_set_enable_verify, every frame held to its own stream's numbering) and exits non-zero with the
 * verifier's message when one does not.
 *
 *   flake_amd_cli --decode in.flac out.wav
 *
 * --decode turns a FLAC file back into canonical PCM WAV on the GPU (flake_amd_decode_*): it checks the "fLaC" marker,
 * reads STREAMINFO, skips the other metadata blocks, finds the frames on the device (flake_amd_decode_index; on the CPU,
 * flake_amd_index_frames, with FLAKE_AMD_INDEX_HOST=1 or for a file of 2 GiB and more), decodes
 * them in batches and compares the MD5 of what it wrote with STREAMINFO's unless that is all zero.  A frame that does
 * not decode, or an MD5 mismatch, ends in a non-zero exit status with the frame named on stderr.
 *
 *   flake_amd_cli --decode --set OUTDIR a.flac b.flac ...
 *
 * --decode --set decodes files of one format through one decode set (flake_amd_decode_set_*): every file is indexed
 * on the CPU, their frames go round-robin into shared GPU batches, every stream's MD5 is carried on the device and
 * held against its STREAMINFO, and OUTDIR/<name>.wav is written per input.  An input whose format differs from the
 * first's is an error that names it.  A file that fails is named on stderr and makes the exit status non-zero; the other
 * files are still written in full.
 *
 *   flake_amd_cli [-0..-12] [-b blocksize] --recode --set OUTDIR [--verify] a.flac b.flac ...
 *
 * --recode --set re-encodes FLAC files of one format at another level through one recode set (flake_amd_recode_set_*):
 * frames found as in --decode --set, decoded, re-cut into the new block size and encoded without the samples leaving
 * the device.  OUTDIR/<name>.flac is "fLaC" + the new STREAMINFO + frames, as the encoder writes it; other metadata
 * blocks are NOT carried over.  A file whose decode fails, or whose digest differs from a non-zero source digest, is
 * named on stderr, gets no output (one left by an earlier run is removed) and makes the exit status non-zero; the
 * other files are written.  --verify turns the recode set's on-device verification on.
 *
 * Only canonical PCM WAV (8/16/24/32 bit) is read; this is a harness for the
 * host API, not a replacement for the reference's libpcm_io.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"

static uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

typedef struct { FILE *f; int channels, rate, bps; uint32_t frames; } wav_t;

static int wav_open(wav_t *w, const char *path)
{
    uint8_t h[12], ck[8];
    w->f = fopen(path, "rb");
    if (!w->f || fread(h, 1, 12, w->f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return -1;
    int have_fmt = 0;
    while (fread(ck, 1, 8, w->f) == 8) {
        uint32_t sz = rd32(ck + 4);
        if (!memcmp(ck, "fmt ", 4)) {
            uint8_t f[40];
            uint32_t take = sz < 40 ? sz : 40;
            if (fread(f, 1, take, w->f) != take) return -1;
            if (sz > take) fseek(w->f, (long)(sz - take), SEEK_CUR);
            int tag = rd16(f);
            if (tag != 1 && tag != 0xFFFE) return -1;
            w->channels = rd16(f + 2); w->rate = (int)rd32(f + 4); w->bps = rd16(f + 14);
            have_fmt = 1;
        } else if (!memcmp(ck, "data", 4)) {
            if (!have_fmt) return -1;
            w->frames = sz / (uint32_t)(w->channels * ((w->bps + 7) / 8));
            return 0;
        } else {
            fseek(w->f, (long)(sz + (sz & 1)), SEEK_CUR);
        }
    }
    return -1;
}

/* up to `frames` sample-frames, sign-extended (pcm_io.c:155-277): interleaved int32 into dst, or -- dst16 given, files
 * of 16 bits per sample or fewer -- interleaved int16 into dst16 */
static uint32_t wav_read(wav_t *w, int32_t *dst, int16_t *dst16, uint32_t frames)
{
    const int bytes = (w->bps + 7) / 8;
    const size_t want = (size_t)frames * w->channels;
    uint8_t *raw = (uint8_t *)malloc(want * bytes);
    size_t got = fread(raw, (size_t)bytes, want, w->f);
    for (size_t i = 0; i < got; i++) {
        const uint8_t *p = raw + i * bytes;
        int32_t v;
        if (bytes == 1) v = (int32_t)p[0] - 128;
        else if (bytes == 2) v = (int16_t)rd16(p);
        else if (bytes == 3) v = (int32_t)((uint32_t)p[0] << 8 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 24) >> 8;
        else v = (int32_t)rd32(p);
        if (dst16) dst16[i] = (int16_t)v; else dst[i] = v;
    }
    free(raw);
    return (uint32_t)(got / w->channels);
}

/* ---- --set: many inputs of one format through one stream set -------- */
typedef struct { uint8_t *p; size_t n, cap; } bytes_t;

static int bytes_add(bytes_t *b, const uint8_t *src, size_t n)
{
    if (b->n + n > b->cap) {
        size_t cap = b->cap ? b->cap * 2 : 65536;
        while (cap < b->n + n) cap *= 2;
        uint8_t *q = (uint8_t *)realloc(b->p, cap);
        if (!q) return -1;
        b->p = q; b->cap = cap;
    }
    memcpy(b->p + b->n, src, n);
    b->n += n;
    return 0;
}

typedef struct {
    FlakeAmdSet *g;
    int sample_bytes, bs, nch, cap_blocks, count;
    char *pcm;                            /* the batch being filled */
    int *stream_of, *sizes;
    uint8_t *buf; size_t buf_cap;
    bytes_t *outs;                        /* per stream: its frames */
} set_run;

static int set_flush(set_run *r, int block_size)
{
    if (!r->count) return 0;
    const long long n = flake_amd_set_encode(r->g, r->pcm, r->sample_bytes, r->count, block_size, r->stream_of,
                                             r->buf, r->buf_cap, r->sizes);
    if (n < 0) { fprintf(stderr, "encode error: %s\n", flake_amd_set_last_error(r->g)); return -1; }
    size_t pos = 0;
    for (int b = 0; b < r->count; b++) {
        if (bytes_add(&r->outs[r->stream_of[b]], r->buf + pos, (size_t)r->sizes[b])) return -1;
        pos += (size_t)r->sizes[b];
    }
    r->count = 0;
    return 0;
}

static int set_add(set_run *r, int stream, const char *block, int block_size)
{
    const size_t bytes = (size_t)block_size * r->nch * r->sample_bytes;
    memcpy(r->pcm + (size_t)r->count * bytes, block, bytes);
    r->stream_of[r->count++] = stream;
    return r->count == r->cap_blocks ? set_flush(r, block_size) : 0;
}

static int run_set(const char *outdir, char **inputs, int ninputs, int synth_streams, int synth, int level, int bsize,
                   int channels, int bps, int verify)
{
    const int S = ninputs ? ninputs : synth_streams;
    FlakeAmdContext s;
    memset(&s, 0, sizeof s);
    wav_t *wavs = (wav_t *)calloc((size_t)S, sizeof(wav_t));
    uint32_t *frames = (uint32_t *)calloc((size_t)S, sizeof(uint32_t));
    char **data = (char **)calloc((size_t)S, sizeof(char *));
    bytes_t *outs = (bytes_t *)calloc((size_t)S, sizeof(bytes_t));
    if (!wavs || !frames || !data || !outs) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i < ninputs; i++) {
        if (wav_open(&wavs[i], inputs[i])) { fprintf(stderr, "cannot read %s as PCM WAV\n", inputs[i]); return 1; }
        if (i && (wavs[i].channels != wavs[0].channels || wavs[i].rate != wavs[0].rate || wavs[i].bps != wavs[0].bps)) {
            fprintf(stderr, "%s: a set's inputs must share channels, sample rate and bits per sample\n", inputs[i]);
            return 1;
        }
    }
    s.channels = ninputs ? wavs[0].channels : channels;
    s.sample_rate = ninputs ? wavs[0].rate : 44100;
    s.bits_per_sample = ninputs ? wavs[0].bps : bps;
    s.params.compression = level;
    if (flake_amd_set_defaults(&s.params)) return 1;
    if (bsize > 0) s.params.block_size = bsize;
    if (flake_amd_validate_params(&s) < 0) { fprintf(stderr, "invalid parameters\n"); return 1; }
    /* (variable block size, levels 9-12: the set takes int32 samples only) */
    const int bs = s.params.block_size, nch = s.channels;
    const int narrow = s.bits_per_sample <= 16 && !s.params.variable_block_size;
    const int sample_bytes = narrow ? 2 : 4;
    /* every input whole in memory (a harness): int16 samples where the files hold 16 bits or fewer */
    for (int i = 0; i < S; i++) {
        frames[i] = ninputs ? wavs[i].frames : (uint32_t)synth * (uint32_t)bs;
        const size_t vals = (size_t)frames[i] * nch;
        data[i] = (char *)malloc((vals ? vals : 1) * sample_bytes);
        int32_t *wide = (!ninputs || !narrow) ? (int32_t *)malloc((vals ? vals : 1) * sizeof(int32_t)) : NULL;
        if (!data[i] || ((!ninputs || !narrow) && !wide)) { fprintf(stderr, "out of memory\n"); return 1; }
        if (ninputs) {
            frames[i] = wav_read(&wavs[i], wide, narrow ? (int16_t *)data[i] : NULL, frames[i]);
            fclose(wavs[i].f);
        } else {
            /* stream i: the synthetic signal from frame index i * FRAMES on, so the streams differ */
            flake_amd_synth_pcm(wide, (int64_t)i * synth, synth, bs, nch, s.bits_per_sample);
        }
        if (wide && narrow) for (size_t k = 0; k < vals; k++) ((int16_t *)data[i])[k] = (int16_t)wide[k];
        else if (wide) memcpy(data[i], wide, (size_t)frames[i] * nch * sizeof(int32_t));
        free(wide);
    }
    /* the stream header of the single-input form (flake.c:558), STREAMINFO rewritten per stream below */
    const int hlen = flake_amd_encode_init(&s);
    if (hlen < 0) { fprintf(stderr, "encoder init failed (%d)\n", hlen); return 1; }
    uint8_t *header = (uint8_t *)malloc((size_t)hlen);
    memcpy(header, s.header, (size_t)hlen);
    flake_amd_encode_close(&s);

    set_run r;
    memset(&r, 0, sizeof r);
    r.g = flake_amd_set_open(&s, S, s.params.variable_block_size ? FLAKE_AMD_SET_VBS : 0);
    if (!r.g) { fprintf(stderr, "%s\n", flake_amd_set_last_error(NULL)); return 1; }
    if (verify && flake_amd_set_enable_verify(r.g, 1)) { fprintf(stderr, "cannot turn verification on\n"); return 1; }
    r.sample_bytes = sample_bytes; r.bs = bs; r.nch = nch; r.cap_blocks = 1024; r.outs = outs;
    r.pcm = (char *)malloc((size_t)r.cap_blocks * bs * nch * sample_bytes);
    r.stream_of = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    r.sizes = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    r.buf_cap = (size_t)r.cap_blocks * bs * nch * 5 + 65536;
    r.buf = (uint8_t *)malloc(r.buf_cap);
    if (!r.pcm || !r.stream_of || !r.sizes || !r.buf) { fprintf(stderr, "out of memory\n"); return 1; }
    const size_t bbytes = (size_t)bs * nch * sample_bytes;
    uint32_t rounds = 0;
    for (int i = 0; i < S; i++) if (frames[i] / (uint32_t)bs > rounds) rounds = frames[i] / (uint32_t)bs;
    for (uint32_t k = 0; k < rounds; k++)                       /* whole blocks, round-robin over the streams */
        for (int i = 0; i < S; i++)
            if (k < frames[i] / (uint32_t)bs && set_add(&r, i, data[i] + (size_t)k * bbytes, bs)) return 1;
    if (set_flush(&r, bs)) return 1;
    /* tails: every stream's last, short block in ONE ragged call (per cap_blocks streams), whatever their lengths */
    int *tail_of = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    if (!tail_of) { fprintf(stderr, "out of memory\n"); return 1; }
    for (int i = 0; i <= S; i++) {
        const int tail = i < S ? (int)(frames[i] % (uint32_t)bs) : 0;
        if (i < S && tail) {
            size_t at = 0;
            for (int b = 0; b < r.count; b++) at += (size_t)tail_of[b] * nch * sample_bytes;
            memcpy(r.pcm + at, data[i] + (size_t)(frames[i] / (uint32_t)bs) * bbytes, (size_t)tail * nch * sample_bytes);
            tail_of[r.count] = tail;
            r.stream_of[r.count++] = i;
        }
        if (r.count && (r.count == r.cap_blocks || i == S)) {
            const long long n = flake_amd_set_encode_ragged(r.g, r.pcm, sample_bytes, r.count, tail_of, r.stream_of, r.buf,
                                                            r.buf_cap, r.sizes);
            if (n < 0) { fprintf(stderr, "encode error: %s\n", flake_amd_set_last_error(r.g)); return 1; }
            size_t pos = 0;
            for (int b = 0; b < r.count; b++) {
                if (bytes_add(&outs[r.stream_of[b]], r.buf + pos, (size_t)r.sizes[b])) return 1;
                pos += (size_t)r.sizes[b];
            }
            r.count = 0;
        }
    }
    free(tail_of);
    unsigned long long total_in = 0, total_out = 0;
    for (int i = 0; i < S; i++) {
        char path[4096];
        if (ninputs) {
            const char *base = strrchr(inputs[i], '/');
            base = base ? base + 1 : inputs[i];
            size_t len = strlen(base);
            if (len > 4 && !strcmp(base + len - 4, ".wav")) len -= 4;
            snprintf(path, sizeof path, "%s/%.*s.flac", outdir, (int)len, base);
        } else {
            snprintf(path, sizeof path, "%s/stream%05d.flac", outdir, i);
        }
        FlakeAmdStreaminfo si;
        if (flake_amd_set_get_streaminfo(r.g, i, &si)) { fprintf(stderr, "%s\n", flake_amd_set_last_error(r.g)); return 1; }
        flake_amd_write_streaminfo(&si, header + 8);            /* flake.c:668-679 */
        FILE *fo = fopen(path, "wb");
        if (!fo) { perror(path); return 1; }
        fwrite(header, 1, (size_t)hlen, fo);
        fwrite(outs[i].p, 1, outs[i].n, fo);
        fclose(fo);
        total_in += frames[i]; total_out += (unsigned long long)hlen + outs[i].n;
        free(outs[i].p); free(data[i]);
    }
    fprintf(stderr, "%d streams, %llu sample-frames -> %llu bytes (ratio %.3f)\n", S, total_in, total_out,
            total_in ? (double)total_out / ((double)total_in * nch * ((s.bits_per_sample + 7) / 8)) : 0.0);
    flake_amd_set_close(r.g);
    free(r.pcm); free(r.stream_of); free(r.sizes); free(r.buf); free(header);
    free(wavs); free(frames); free(data); free(outs);
    return 0;
}

/* ---- --decode: a FLAC file back to canonical PCM WAV ----------------- */
static void wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

static void wav_header(uint8_t h[44], int channels, int rate, int bps, uint32_t frames)
{
    const int bytes = (bps + 7) / 8;
    const uint32_t data = frames * (uint32_t)(channels * bytes);
    memcpy(h, "RIFF", 4); wr32(h + 4, 36 + data); memcpy(h + 8, "WAVEfmt ", 8); wr32(h + 16, 16);
    h[20] = 1; h[21] = 0; h[22] = (uint8_t)channels; h[23] = 0;
    wr32(h + 24, (uint32_t)rate); wr32(h + 28, (uint32_t)(rate * channels * bytes));
    h[32] = (uint8_t)(channels * bytes); h[33] = 0; h[34] = (uint8_t)bps; h[35] = 0;
    memcpy(h + 36, "data", 4); wr32(h + 40, data);
}

/* FLAKE_AMD_INDEX_HOST=1: frame discovery stays on the CPU (flake_amd_index_frames) */
static int index_on_host(void)
{
    const char *e = getenv("FLAKE_AMD_INDEX_HOST");
    return e && *e && strcmp(e, "0");
}

static int run_decode(const char *in, const char *out)
{
    FILE *fi = fopen(in, "rb");
    if (!fi) { perror(in); return 1; }
    fseek(fi, 0, SEEK_END);
    const long flen = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    uint8_t *file = (uint8_t *)malloc(flen > 0 ? (size_t)flen : 1);          /* the file whole in memory (a harness) */
    if (!file || flen < 0 || fread(file, 1, (size_t)flen, fi) != (size_t)flen) { fprintf(stderr, "cannot read %s\n", in); return 1; }
    fclose(fi);
    const size_t len = (size_t)flen;
    if (len < 4 + 4 + 34 || memcmp(file, "fLaC", 4) || (file[4] & 0x7F) != 0 ||
        ((size_t)file[5] << 16 | (size_t)file[6] << 8 | file[7]) != 34) {
        fprintf(stderr, "%s: not a FLAC file (no fLaC marker followed by STREAMINFO)\n", in);
        return 1;
    }
    FlakeAmdStreaminfo si;
    if (flake_amd_read_streaminfo(file + 8, &si) < 0) { fprintf(stderr, "%s: invalid STREAMINFO\n", in); return 1; }
    size_t pos = 4;
    for (;;) {                                                               /* skip every metadata block */
        if (pos + 4 > len) { fprintf(stderr, "%s: metadata runs past the file\n", in); return 1; }
        const int last = file[pos] >> 7;
        pos += 4 + ((size_t)file[pos + 1] << 16 | (size_t)file[pos + 2] << 8 | file[pos + 3]);
        if (pos > len) { fprintf(stderr, "%s: metadata runs past the file\n", in); return 1; }
        if (last) break;
    }
    FlakeAmdDecoder *d = flake_amd_decode_open(&si);
    if (!d) { fprintf(stderr, "decoder init failed: %s\n", flake_amd_decode_last_error(NULL)); return 1; }
    FILE *fo = fopen(out, "wb");
    if (!fo) { perror(out); return 1; }
    const int nch = (int)si.channels, bps = (int)si.bits_per_sample, wbytes = (bps + 7) / 8;
    const int narrow = bps == 16;                                            /* int16 all the way (the 2-byte path) */
    const int maxn = si.max_block_size ? (int)si.max_block_size : 65535;
    const int batch = (4 << 20) / maxn < 1024 ? (4 << 20) / maxn : 1024;     /* frames per round: about 4M samples */
    int *sizes = (int *)malloc(sizeof(int) * (size_t)batch);
    const size_t cap = (size_t)batch * (size_t)maxn;
    void *pcm = malloc(cap * (size_t)nch * (narrow ? 2 : 4));
    uint8_t *raw = (uint8_t *)malloc(cap * (size_t)nch * (size_t)wbytes);
    if (!sizes || !pcm || !raw) { fprintf(stderr, "out of memory\n"); return 1; }
    uint8_t wh[44];
    memset(wh, 0, sizeof wh);
    fwrite(wh, 1, 44, fo);
    unsigned long long total = 0, nframes_done = 0;
    int rc = 0;
    /* the frames of the whole file, found on the device in one call (K8): the same frames as the CPU finds piece by
     * piece below, since a piece's last frame ends at the header the next piece begins with.  FLAKE_AMD_INDEX_HOST=1,
     * or a file the device indexer refuses (2 GiB and more), keeps the CPU */
    int *all = NULL;
    long long all_n = 0, all_next = 0;
    int on_device = 0;
    if (!index_on_host() && pos < len && len - pos < ((size_t)1 << 31)) {
        const int all_cap = (int)((len - pos) / 8 + 1);
        size_t all_used = 0;
        all = (int *)malloc(sizeof(int) * (size_t)all_cap);
        all_n = all ? flake_amd_decode_index(d, file + pos, len - pos, all, all_cap, &all_used) : -2;
        on_device = all_n != -2;
    }
    while (pos < len) {
        size_t used = 0;
        long long nf;
        if (on_device) {
            nf = all_n < 0 ? -1 : (all_n - all_next < batch ? all_n - all_next : batch);
            for (long long k = 0; k < nf; k++) { sizes[k] = all[all_next + k]; used += (size_t)sizes[k]; }
            if (nf > 0) all_next += nf;
        } else {
            nf = flake_amd_index_frames(&si, file + pos, len - pos, sizes, batch, &used);
        }
        if (nf <= 0) {
            fprintf(stderr, "%s: frame %llu (at byte %llu, after %llu samples): %s\n", in, nframes_done,
                    (unsigned long long)pos, total,
                    nf < 0 ? "not a frame header of this stream" : "the frame is cut or its CRC-16 fails");
            rc = 1;
            break;
        }
        const long long ns = flake_amd_decode_frames(d, file + pos, used, sizes, (int)nf, pcm, narrow ? 2 : 4, cap);
        if (ns < 0) { fprintf(stderr, "decode error: %s\n", flake_amd_decode_last_error(d)); rc = 1; break; }
        const size_t vals = (size_t)ns * (size_t)nch;
        if (narrow) {
            fwrite(pcm, 2, vals, fo);                                        /* (little-endian hosts, as the reader) */
        } else {
            const int32_t *v = (const int32_t *)pcm;
            for (size_t i = 0; i < vals; i++) {
                const uint32_t u = wbytes == 1 ? (uint32_t)(v[i] + 128) : (uint32_t)v[i];
                for (int b = 0; b < wbytes; b++) raw[i * (size_t)wbytes + (size_t)b] = (uint8_t)(u >> (8 * b));
            }
            fwrite(raw, (size_t)wbytes, vals, fo);
        }
        total += (unsigned long long)ns;
        nframes_done += (unsigned long long)nf;
        pos += used;
    }
    wav_header(wh, nch, (int)si.sample_rate, bps, (uint32_t)total);
    fseek(fo, 0, SEEK_SET);
    fwrite(wh, 1, 44, fo);
    fclose(fo);
    if (!rc) {
        static const uint8_t zero[16] = {0};
        uint8_t md5[16];
        flake_amd_decode_md5(d, md5);
        if (memcmp(si.md5sum, zero, 16) && memcmp(si.md5sum, md5, 16)) {
            fprintf(stderr, "%s: MD5 mismatch: the decoded samples are not what STREAMINFO's signature was made of\n", in);
            rc = 1;
        } else if (si.samples && (unsigned long long)si.samples != (total & 0xFFFFFFFFull)) {
            fprintf(stderr, "%s: %llu samples decoded, STREAMINFO says %u\n", in, total, si.samples);
            rc = 1;
        }
    }
    if (!rc) fprintf(stderr, "%llu sample-frames decoded\n", total);
    flake_amd_decode_close(d);
    free(file); free(sizes); free(pcm); free(raw); free(all);
    return rc;
}

/* ---- --decode --set: many FLAC files of one format through one decode set ---- */
typedef struct {
    const char *path;
    uint8_t *file;
    size_t len, pos;                 /* the file, and where its next frame starts */
    FlakeAmdStreaminfo si;
    int *sizes;                      /* every frame's size (the indexer's, over the whole file) */
    int own_sizes;                   /* ... in a block of the file's own (the CPU indexer's), not in the group's */
    long long nframes, next;         /* ... how many, and the next one to hand over */
    FILE *fo;
    unsigned long long total;
    int bad;                         /* named on stderr already */
    int skip;                        /* ... before it was a stream at all: it has no output file */
    char name[1024];                 /* OUTDIR/<name>.wav */
} dset_file;

static void dset_free(dset_file *fs, int n)
{
    for (int i = 0; i < n; i++) {
        if (fs[i].fo) fclose(fs[i].fo);
        free(fs[i].file);
        if (fs[i].own_sizes) free(fs[i].sizes);
    }
    free(fs);
}

static int dset_load(dset_file *f)
{
    FILE *fi = fopen(f->path, "rb");
    if (!fi) { perror(f->path); return 1; }
    fseek(fi, 0, SEEK_END);
    const long flen = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    f->file = (uint8_t *)malloc(flen > 0 ? (size_t)flen : 1);
    if (!f->file || flen < 0 || fread(f->file, 1, (size_t)flen, fi) != (size_t)flen) { fprintf(stderr, "cannot read %s\n", f->path); fclose(fi); return 1; }
    fclose(fi);
    f->len = (size_t)flen;
    if (f->len < 4 + 4 + 34 || memcmp(f->file, "fLaC", 4) || (f->file[4] & 0x7F) != 0 ||
        ((size_t)f->file[5] << 16 | (size_t)f->file[6] << 8 | f->file[7]) != 34) {
        fprintf(stderr, "%s: not a FLAC file (no fLaC marker followed by STREAMINFO)\n", f->path);
        return 1;
    }
    if (flake_amd_read_streaminfo(f->file + 8, &f->si) < 0) { fprintf(stderr, "%s: invalid STREAMINFO\n", f->path); return 1; }
    size_t pos = 4;
    for (;;) {
        if (pos + 4 > f->len) { fprintf(stderr, "%s: metadata runs past the file\n", f->path); return 1; }
        const int last = f->file[pos] >> 7;
        pos += 4 + ((size_t)f->file[pos + 1] << 16 | (size_t)f->file[pos + 2] << 8 | f->file[pos + 3]);
        if (pos > f->len) { fprintf(stderr, "%s: metadata runs past the file\n", f->path); return 1; }
        if (last) break;
    }
    f->pos = pos;
    return 0;
}

static int run_decode_set(const char *outdir, char **inputs, int n)
{
    if (n < 1) { fprintf(stderr, "--decode --set needs input files\n"); return 2; }
    dset_file *fs = (dset_file *)calloc((size_t)n, sizeof *fs);
    if (!fs) return 1;
    int rc = 0, ref = -1;
    unsigned maxn = 16;
    /* a file that cannot be read or is no FLAC file is named (dset_load) and left out, like one that fails later; the
     * first one that loads sets the format */
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        f->path = inputs[i];
        if (dset_load(f)) {
            f->bad = f->skip = 1;
            rc = 1;
            continue;
        }
        if (ref < 0) ref = i;
        if (f->si.channels != fs[ref].si.channels || f->si.bits_per_sample != fs[ref].si.bits_per_sample ||
            f->si.sample_rate != fs[ref].si.sample_rate) {
            fprintf(stderr, "%s: its format (%u channels, %u bits, %u Hz) differs from %s's: a decode set takes one format\n",
                    f->path, f->si.channels, f->si.bits_per_sample, f->si.sample_rate, fs[ref].path);
            dset_free(fs, n);
            return 1;
        }
        const unsigned mb = f->si.max_block_size ? f->si.max_block_size : 65535u;
        if (mb > maxn) maxn = mb;
        const char *base = strrchr(f->path, '/');
        base = base ? base + 1 : f->path;
        const char *dot = strrchr(base, '.');
        snprintf(f->name, sizeof f->name, "%s/%.*s.wav", outdir, (int)(dot ? dot - base : (long)strlen(base)), base);
        for (int j = 0; j < i; j++)
            if (!fs[j].skip && !strcmp(fs[j].name, f->name)) {
                fprintf(stderr, "%s and %s would both be written to %s\n", fs[j].path, f->path, f->name);
                dset_free(fs, n);
                return 1;
            }
    }
    if (ref < 0) { dset_free(fs, n); return 1; }
    FlakeAmdStreaminfo like = fs[ref].si;
    like.max_block_size = maxn;
    const int nch = (int)like.channels, bps = (int)like.bits_per_sample, wbytes = (bps + 7) / 8, narrow = bps == 16;
    /* (everything the loops below need, so that every way out frees it) */
    int *sor = NULL, *fof = NULL, *csz = NULL, *group_sizes = NULL;
    long long *rs = NULL, *ro = NULL;
    void *pcm = NULL;
    uint8_t *raw = NULL, *bytes = NULL;
    size_t bytes_cap = 0;
    FlakeAmdDecodeSet *g = flake_amd_decode_set_open(&like, n, 0);
    if (!g) { fprintf(stderr, "decode set init failed: %s\n", flake_amd_decode_set_last_error(NULL)); rc = 1; goto out; }
    /* the frames of every file, found on the device (K8): all files in one call, as ranges of one buffer, while they
     * stay below 2 GiB together.  FLAKE_AMD_INDEX_HOST=1, a device that cannot answer, or what is left over, goes to
     * the CPU file by file */
    size_t *used_of = (size_t *)calloc((size_t)n, sizeof(size_t));
    char *indexed = (char *)calloc((size_t)n, 1);
    if (!used_of || !indexed) { fprintf(stderr, "out of memory\n"); free(used_of); free(indexed); rc = 1; goto out; }
    char *tried = (char *)calloc((size_t)n, 1);
    if (!tried) { fprintf(stderr, "out of memory\n"); free(used_of); free(indexed); rc = 1; goto out; }
    long long group_at = 0, group_cap = 0;
    for (int i = 0; i < n && !index_on_host(); i++) group_cap += fs[i].skip ? 0 : (long long)((fs[i].len - fs[i].pos) / 8 + 2);
    if (group_cap) group_sizes = (int *)malloc(sizeof(int) * (size_t)group_cap);
    /* one call per max_block_size among the files (a call holds one format): as a rule, one call */
    for (int lead = 0; lead < n && group_sizes; lead++) {
        if (fs[lead].skip || tried[lead]) continue;
        const unsigned mbs = fs[lead].si.max_block_size;
        size_t tot = 0;
        int members = 0;
        for (int i = lead; i < n; i++) {
            const size_t left = fs[i].len - fs[i].pos;
            if (fs[i].skip || tried[i] || fs[i].si.max_block_size != mbs || tot + left >= ((size_t)1 << 31)) continue;
            tried[i] = 2;
            tot += left;
            members++;
        }
        size_t *first = (size_t *)malloc(sizeof(size_t) * ((size_t)members + 1));
        long long *frames = (long long *)malloc(sizeof(long long) * ((size_t)members + 1));
        size_t *cons = (size_t *)malloc(sizeof(size_t) * ((size_t)members + 1));
        if (tot > bytes_cap) {
            free(bytes);
            bytes = (uint8_t *)malloc(tot);
            bytes_cap = bytes ? tot : 0;
        }
        int ok = members > 0 && first && frames && cons && (bytes || !tot);
        if (ok) {
            size_t at = 0;
            int r = 0;
            for (int i = lead; i < n; i++) {
                if (tried[i] != 2) continue;
                first[r++] = at;
                if (fs[i].len > fs[i].pos) memcpy(bytes + at, fs[i].file + fs[i].pos, fs[i].len - fs[i].pos);
                at += fs[i].len - fs[i].pos;
            }
            first[r] = at;
            ok = flake_amd_decode_set_index(g, mbs, bytes, first, members, group_sizes + group_at, (int)(tot / 8) + members + 1,
                                            frames, cons) == 0;
        }
        int r = 0;
        for (int i = lead; i < n; i++) {
            if (tried[i] != 2) continue;
            tried[i] = 1;
            if (ok) {
                indexed[i] = 1;
                fs[i].sizes = group_sizes + group_at;
                fs[i].nframes = frames[r];
                used_of[i] = cons[r];
                if (frames[r] > 0) group_at += frames[r];
            }
            r++;
        }
        free(first); free(frames); free(cons);
    }
    free(tried);
    /* a file whose frames end early is named now and decoded up to there */
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        if (f->skip) continue;
        const size_t left = f->len - f->pos;
        size_t used = used_of[i];
        if (!indexed[i]) {
            const int cap = (int)(left / 8 + 1);
            f->sizes = (int *)malloc(sizeof(int) * (size_t)cap);
            f->own_sizes = 1;
            f->nframes = f->sizes ? flake_amd_index_frames(&f->si, f->file + f->pos, left, f->sizes, cap, &used) : -1;
        }
        if (f->nframes < 0 || used != left) {
            fprintf(stderr, "%s: frame %lld (at byte %llu): %s\n", f->path, f->nframes < 0 ? 0ll : f->nframes,
                    (unsigned long long)(f->pos + used), f->nframes < 0 ? "not a frame header of this stream" : "the frame is cut or its CRC-16 fails");
            f->bad = 1;
            rc = 1;
            if (f->nframes < 0) f->nframes = 0;
        }
        f->fo = fopen(f->name, "wb");
        if (!f->fo) { perror(f->name); free(used_of); free(indexed); rc = 1; goto out; }
        uint8_t wh[44];
        memset(wh, 0, sizeof wh);
        fwrite(wh, 1, 44, f->fo);
    }
    free(used_of); free(indexed);
    /* round-robin: a call takes up to `per` frames of every file that has some left */
    int per = (int)((4u << 20) / maxn / (unsigned)n);
    if (per > 64) per = 64;
    if (per < 1) per = 1;
    sor = (int *)malloc(sizeof(int) * (size_t)n);
    fof = (int *)malloc(sizeof(int) * (size_t)n);
    csz = (int *)malloc(sizeof(int) * (size_t)n * (size_t)per);
    rs = (long long *)malloc(sizeof(long long) * (size_t)n);
    ro = (long long *)malloc(sizeof(long long) * (size_t)n);
    const size_t cap = (size_t)n * (size_t)per * (size_t)maxn;
    pcm = malloc(cap * (size_t)nch * (narrow ? 2 : 4));
    raw = (uint8_t *)malloc((size_t)per * (size_t)maxn * (size_t)nch * (size_t)wbytes);
    if (!sor || !fof || !csz || !rs || !ro || !pcm || !raw) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
    for (;;) {
        int nruns = 0, nfr = 0;
        size_t nb = 0;
        for (int i = 0; i < n; i++) {
            dset_file *f = &fs[i];
            if (f->skip || f->next >= f->nframes || flake_amd_decode_set_failed(g, i, NULL, NULL) == 1) continue;
            const int take = f->nframes - f->next < per ? (int)(f->nframes - f->next) : per;
            size_t rb = 0;
            for (int k = 0; k < take; k++) { csz[nfr++] = f->sizes[f->next + k]; rb += (size_t)f->sizes[f->next + k]; }
            if (nb + rb > bytes_cap) {
                uint8_t *more = (uint8_t *)realloc(bytes, (nb + rb) * 2);
                if (!more) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
                bytes = more;
                bytes_cap = (nb + rb) * 2;
            }
            memcpy(bytes + nb, f->file + f->pos, rb);
            nb += rb;
            f->pos += rb;
            f->next += take;
            sor[nruns] = i;
            fof[nruns++] = take;
        }
        if (!nruns) break;
        if (flake_amd_decode_set_frames(g, nruns, sor, fof, bytes, nb, csz, pcm, narrow ? 2 : 4, cap, rs) < 0 ||
            flake_amd_decode_set_run_offsets(g, ro, nruns) != nruns) {
            fprintf(stderr, "decode error: %s\n", flake_amd_decode_set_last_error(g));
            rc = 1;
            goto out;
        }
        for (int r = 0; r < nruns; r++) {
            dset_file *f = &fs[sor[r]];
            if (rs[r] < 0) {
                long long fr = -1;
                int st = 0;
                flake_amd_decode_set_failed(g, sor[r], &fr, &st);
                fprintf(stderr, "%s: frame %lld does not decode (status %d)\n", f->path, fr, st);
                f->bad = 1;
                rc = 1;
                continue;
            }
            const size_t vals = (size_t)rs[r] * (size_t)nch;
            if (narrow) {
                fwrite((const int16_t *)pcm + (size_t)ro[r] * (size_t)nch, 2, vals, f->fo);
            } else {
                const int32_t *v = (const int32_t *)pcm + (size_t)ro[r] * (size_t)nch;
                for (size_t i = 0; i < vals; i++) {
                    const uint32_t u = wbytes == 1 ? (uint32_t)(v[i] + 128) : (uint32_t)v[i];
                    for (int b = 0; b < wbytes; b++) raw[i * (size_t)wbytes + (size_t)b] = (uint8_t)(u >> (8 * b));
                }
                fwrite(raw, (size_t)wbytes, vals, f->fo);
            }
            f->total += (unsigned long long)rs[r];
        }
    }
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        if (f->skip) continue;
        uint8_t wh[44];
        wav_header(wh, nch, (int)like.sample_rate, bps, (uint32_t)f->total);
        fseek(f->fo, 0, SEEK_SET);
        fwrite(wh, 1, 44, f->fo);
        if (!f->bad) {
            static const uint8_t zero[16] = {0};
            uint8_t md5[16];
            if (flake_amd_decode_set_md5(g, i, md5) != 0) {
                fprintf(stderr, "%s: %s\n", f->path, flake_amd_decode_set_last_error(g));
                f->bad = 1;
            } else if (memcmp(f->si.md5sum, zero, 16) && memcmp(f->si.md5sum, md5, 16)) {
                fprintf(stderr, "%s: MD5 mismatch: the decoded samples are not what STREAMINFO's signature was made of\n", f->path);
                f->bad = 1;
            } else if (f->si.samples && (unsigned long long)f->si.samples != (f->total & 0xFFFFFFFFull)) {
                fprintf(stderr, "%s: %llu samples decoded, STREAMINFO says %u\n", f->path, f->total, f->si.samples);
                f->bad = 1;
            }
            if (f->bad) rc = 1;
        }
        if (!f->bad) fprintf(stderr, "%s: %llu sample-frames decoded\n", f->path, f->total);
    }
    fprintf(stderr, "%lld device batches\n", flake_amd_decode_set_device_batches(g));
out:
    if (g) flake_amd_decode_set_close(g);
    free(sor); free(fof); free(csz); free(rs); free(ro); free(pcm); free(raw); free(bytes); free(group_sizes);
    dset_free(fs, n);
    return rc;
}

/* ---- --recode --set: many FLAC files of one format re-encoded through one recode set ---- */
#define RECODE_USAGE "usage: %s [-0..-12] [-b blocksize] --recode --set OUTDIR [--verify] a.flac b.flac ...\n" \
                     "       (files of one format; only STREAMINFO is written: other metadata blocks are not carried over)\n"

static int run_recode_set(const char *outdir, char **inputs, int n, int level, int bsize, int verify)
{
    if (n < 1) { fprintf(stderr, "--recode --set needs input files\n"); return 2; }
    dset_file *fs = (dset_file *)calloc((size_t)n, sizeof *fs);
    bytes_t *outs = (bytes_t *)calloc((size_t)n, sizeof *outs);
    if (!fs || !outs) { free(fs); free(outs); return 1; }
    int rc = 0, ref = -1;
    unsigned maxn = 16;
    int *sor = NULL, *fof = NULL, *csz = NULL, *bstream = NULL, *bbytes = NULL;
    uint8_t *bytes = NULL, *obuf = NULL, *header = NULL;
    size_t bytes_cap = 0, obuf_cap = 0;
    int bcap = 0, hlen = 0;
    FlakeAmdDecodeSet *ix = NULL;
    FlakeAmdRecodeSet *g = NULL;
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        f->path = inputs[i];
        if (dset_load(f)) { f->bad = f->skip = 1; rc = 1; continue; }
        if (ref < 0) ref = i;
        if (f->si.channels != fs[ref].si.channels || f->si.bits_per_sample != fs[ref].si.bits_per_sample ||
            f->si.sample_rate != fs[ref].si.sample_rate) {
            fprintf(stderr, "%s: its format (%u channels, %u bits, %u Hz) differs from %s's: a recode set takes one format\n",
                    f->path, f->si.channels, f->si.bits_per_sample, f->si.sample_rate, fs[ref].path);
            rc = 1;
            goto out;
        }
        const unsigned mb = f->si.max_block_size ? f->si.max_block_size : 65535u;
        if (mb > maxn) maxn = mb;
        const char *base = strrchr(f->path, '/');
        base = base ? base + 1 : f->path;
        const char *dot = strrchr(base, '.');
        snprintf(f->name, sizeof f->name, "%s/%.*s.flac", outdir, (int)(dot ? dot - base : (long)strlen(base)), base);
        for (int j = 0; j < i; j++)
            if (!fs[j].skip && !strcmp(fs[j].name, f->name)) {
                fprintf(stderr, "%s and %s would both be written to %s\n", fs[j].path, f->path, f->name);
                rc = 1;
                goto out;
            }
    }
    if (ref < 0) { rc = 1; goto out; }
    FlakeAmdStreaminfo like = fs[ref].si;
    like.max_block_size = maxn;
    /* the encoder's parameters, and the stream header of the single-input form with STREAMINFO rewritten per file */
    FlakeAmdContext s;
    memset(&s, 0, sizeof s);
    s.channels = (int)like.channels; s.sample_rate = (int)like.sample_rate; s.bits_per_sample = (int)like.bits_per_sample;
    s.params.compression = level;
    if (flake_amd_set_defaults(&s.params)) { rc = 1; goto out; }
    if (bsize > 0) s.params.block_size = bsize;
    if (flake_amd_validate_params(&s) < 0) { fprintf(stderr, "invalid parameters\n"); rc = 1; goto out; }
    hlen = flake_amd_encode_init(&s);
    if (hlen < 0) { fprintf(stderr, "encoder init failed (%d)\n", hlen); rc = 1; goto out; }
    header = (uint8_t *)malloc((size_t)hlen);
    if (header) memcpy(header, s.header, (size_t)hlen);
    flake_amd_encode_close(&s);
    if (!header) { rc = 1; goto out; }
    /* the frames of every file, found on the device (K8) through a decode set's handle; on the CPU with
     * FLAKE_AMD_INDEX_HOST=1 or where the device cannot answer */
    if (!index_on_host()) ix = flake_amd_decode_set_open(&like, 1, FLAKE_AMD_SET_MD5_OFF);
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        if (f->skip) continue;
        const size_t left = f->len - f->pos;
        const int cap = (int)(left / 8 + 2);
        size_t used = 0;
        f->sizes = (int *)malloc(sizeof(int) * (size_t)cap);
        f->own_sizes = 1;
        if (!f->sizes) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
        const size_t first[2] = {0, left};
        long long nf = -1;
        if (!ix || left >= ((size_t)1 << 31) ||
            flake_amd_decode_set_index(ix, f->si.max_block_size, f->file + f->pos, first, 1, f->sizes, cap, &nf, &used) != 0)
            nf = flake_amd_index_frames(&f->si, f->file + f->pos, left, f->sizes, cap, &used);
        f->nframes = nf;
        if (nf < 0 || used != left) {
            fprintf(stderr, "%s: frame %lld (at byte %llu): %s\n", f->path, nf < 0 ? 0ll : nf, (unsigned long long)(f->pos + used),
                    nf < 0 ? "not a frame header of this stream" : "the frame is cut or its CRC-16 fails");
            f->bad = 1;
            rc = 1;
            if (nf < 0) f->nframes = 0;
        }
    }
    if (ix) { flake_amd_decode_set_close(ix); ix = NULL; }
    g = flake_amd_recode_set_open(&like, &s, n, s.params.variable_block_size ? FLAKE_AMD_SET_VBS : 0);
    if (!g) { fprintf(stderr, "recode set init failed: %s\n", flake_amd_recode_set_last_error(NULL)); rc = 1; goto out; }
    if (verify && flake_amd_recode_set_enable_verify(g, 1)) { fprintf(stderr, "cannot turn verification on\n"); rc = 1; goto out; }
    int per = (int)((4u << 20) / maxn / (unsigned)n);
    if (per > 64) per = 64;
    if (per < 1) per = 1;
    sor = (int *)malloc(sizeof(int) * (size_t)n);
    fof = (int *)malloc(sizeof(int) * (size_t)n);
    csz = (int *)malloc(sizeof(int) * (size_t)n * (size_t)per);
    if (!sor || !fof || !csz) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
    for (int last = 0; !last;) {
        int nruns = 0, nfr = 0, nb = 0;
        size_t nbytes = 0;
        for (int i = 0; i < n; i++) {
            dset_file *f = &fs[i];
            if (f->skip || f->next >= f->nframes || flake_amd_recode_set_failed(g, i, NULL, NULL) == 1) continue;
            const int take = f->nframes - f->next < per ? (int)(f->nframes - f->next) : per;
            size_t rb = 0;
            for (int k = 0; k < take; k++) { csz[nfr++] = f->sizes[f->next + k]; rb += (size_t)f->sizes[f->next + k]; }
            if (nbytes + rb > bytes_cap) {
                uint8_t *more = (uint8_t *)realloc(bytes, (nbytes + rb) * 2);
                if (!more) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
                bytes = more;
                bytes_cap = (nbytes + rb) * 2;
            }
            memcpy(bytes + nbytes, f->file + f->pos, rb);
            nbytes += rb;
            f->pos += rb;
            f->next += take;
            sor[nruns] = i;
            fof[nruns++] = take;
        }
        last = !nruns;                     /* no frames left: the tails */
        size_t need = 0;
        long long need_blocks = 0;
        flake_amd_recode_set_out_bound(g, last ? -1 : nfr, &need, &need_blocks);
        if (need > obuf_cap || need_blocks > bcap) {
            free(obuf); free(bstream); free(bbytes);
            obuf_cap = need + 65536;
            bcap = (int)need_blocks + 1024;
            obuf = (uint8_t *)malloc(obuf_cap);
            bstream = (int *)malloc(sizeof(int) * (size_t)bcap);
            bbytes = (int *)malloc(sizeof(int) * (size_t)bcap);
            if (!obuf || !bstream || !bbytes) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
        }
        const long long w = last ? flake_amd_recode_set_finish(g, obuf, obuf_cap, bstream, bbytes, bcap, &nb)
                                 : flake_amd_recode_set_frames(g, nruns, sor, fof, bytes, nbytes, csz, obuf, obuf_cap, bstream,
                                                               bbytes, bcap, &nb);
        if (w < 0) { fprintf(stderr, "recode error: %s\n", flake_amd_recode_set_last_error(g)); rc = 1; goto out; }
        size_t at = 0;
        for (int b = 0; b < nb; b++) {
            if (bytes_add(&outs[bstream[b]], obuf + at, (size_t)bbytes[b])) { fprintf(stderr, "out of memory\n"); rc = 1; goto out; }
            at += (size_t)bbytes[b];
        }
    }
    for (int i = 0; i < n; i++) {
        dset_file *f = &fs[i];
        if (f->skip) continue;
        long long fr = -1;
        int st = 0;
        FlakeAmdStreaminfo si;
        static const uint8_t zero[16] = {0};
        memset(&si, 0, sizeof si);
        if (flake_amd_recode_set_failed(g, i, &fr, &st) == 1) {
            fprintf(stderr, "%s: frame %lld does not decode (status %d)\n", f->path, fr, st);
            f->bad = 1;
        } else if (!f->bad && flake_amd_recode_set_get_streaminfo(g, i, &si)) {
            fprintf(stderr, "%s: %s\n", f->path, flake_amd_recode_set_last_error(g));
            f->bad = 1;
        } else if (!f->bad && memcmp(f->si.md5sum, zero, 16) && memcmp(f->si.md5sum, si.md5sum, 16)) {
            fprintf(stderr, "%s: MD5 mismatch: the decoded samples are not what STREAMINFO's signature was made of\n", f->path);
            f->bad = 1;
        } else if (!f->bad && f->si.samples && f->si.samples != si.samples) {
            fprintf(stderr, "%s: %u samples decoded, STREAMINFO says %u\n", f->path, si.samples, f->si.samples);
            f->bad = 1;
        }
        if (f->bad) {
            /* named above; it gets no output, and one from an earlier run does not stay in its place */
            remove(f->name);
            rc = 1;
            continue;
        }
        flake_amd_write_streaminfo(&si, header + 8);
        FILE *fo = fopen(f->name, "wb");
        if (!fo) { perror(f->name); rc = 1; continue; }
        fwrite(header, 1, (size_t)hlen, fo);
        fwrite(outs[i].p, 1, outs[i].n, fo);
        fclose(fo);
        fprintf(stderr, "%s: %u sample-frames -> %llu bytes\n", f->path, si.samples, (unsigned long long)hlen + outs[i].n);
    }
    {
        long long db = 0, eb = 0;
        flake_amd_recode_set_device_batches(g, &db, &eb);
        fprintf(stderr, "%lld decode batches, %lld encode batches\n", db, eb);
    }
out:
    if (ix) flake_amd_decode_set_close(ix);
    if (g) flake_amd_recode_set_close(g);
    for (int i = 0; i < n; i++) free(outs[i].p);
    free(outs); free(sor); free(fof); free(csz); free(bstream); free(bbytes); free(bytes); free(obuf); free(header);
    dset_free(fs, n);
    return rc;
}

int main(int argc, char **argv)
{
    FlakeAmdContext s;
    memset(&s, 0, sizeof s);
    int level = 5, bsize = -1, synth = 0, channels = 2, bps = 16, verify = 0, synth_streams = 0;
    const char *in = NULL, *out = NULL, *setdir = NULL;
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--recode")) continue;
        /* --recode --set OUTDIR a.flac b.flac ...: everything that is neither switch nor OUTDIR is an input */
        char **inputs = (char **)calloc((size_t)argc, sizeof(char *));
        int ninputs = 0;
        for (int k = 1; k < argc && inputs; k++) {
            if (k == i) continue;
            if (argv[k][0] == '-' && argv[k][1] >= '0' && argv[k][1] <= '9') level = atoi(argv[k] + 1);
            else if (!strcmp(argv[k], "-b") && k + 1 < argc) bsize = atoi(argv[++k]);
            else if (!strcmp(argv[k], "--set") && k + 1 < argc) setdir = argv[++k];
            else if (!strcmp(argv[k], "--verify")) verify = 1;
            else inputs[ninputs++] = argv[k];
        }
        if (!inputs || !setdir || !ninputs) { fprintf(stderr, RECODE_USAGE, argv[0]); free(inputs); return 2; }
        const int rcs = run_recode_set(setdir, inputs, ninputs, level, bsize, verify);
        free(inputs);
        return rcs;
    }
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--decode")) continue;
        for (int j = 1; j + 1 < argc; j++) {
            if (strcmp(argv[j], "--set")) continue;
            /* --decode --set OUTDIR a.flac b.flac ...: everything that is neither switch nor OUTDIR is an input */
            char **inputs = (char **)calloc((size_t)argc, sizeof(char *));
            int ninputs = 0;
            for (int k = 1; k < argc && inputs; k++)
                if (k != i && k != j && k != j + 1) inputs[ninputs++] = argv[k];
            const int rcs = inputs ? run_decode_set(argv[j + 1], inputs, ninputs) : 1;
            free(inputs);
            return rcs;
        }
        if (argc != 4) { fprintf(stderr, "usage: %s --decode in.flac out.wav\n       %s --decode --set OUTDIR a.flac b.flac ...\n", argv[0], argv[0]); return 2; }
        return run_decode(argv[i == 1 ? 2 : 1], argv[i == 3 ? 2 : 3]);
    }
    for (int i = 1; i < argc; i++) if (!strcmp(argv[i], "--set")) setdir = "";
    if (setdir) {
        char **inputs = (char **)calloc((size_t)argc, sizeof(char *));
        int ninputs = 0;
        setdir = NULL;
        for (int i = 1; i < argc; i++) {
            if (argv[i][0] == '-' && argv[i][1] >= '0' && argv[i][1] <= '9') level = atoi(argv[i] + 1);
            else if (!strcmp(argv[i], "-b") && i + 1 < argc) bsize = atoi(argv[++i]);
            else if (!strcmp(argv[i], "--set") && i + 1 < argc) setdir = argv[++i];
            else if (!strcmp(argv[i], "--synth") && i + 1 < argc) synth = atoi(argv[++i]);
            else if (!strcmp(argv[i], "--synth-streams") && i + 1 < argc) synth_streams = atoi(argv[++i]);
            else if (!strcmp(argv[i], "--channels") && i + 1 < argc) channels = atoi(argv[++i]);
            else if (!strcmp(argv[i], "--bps") && i + 1 < argc) bps = atoi(argv[++i]);
            else if (!strcmp(argv[i], "--verify")) verify = 1;
            else inputs[ninputs++] = argv[i];
        }
        if (!setdir || (!ninputs && (synth_streams < 1 || synth < 1)) || (ninputs && synth_streams)) {
            fprintf(stderr, "usage: %s [-0..-12] [-b blocksize] --set OUTDIR [--verify] (in1.wav in2.wav ... | --synth-streams S --synth FRAMES [--channels C] [--bps B])\n", argv[0]);
            return 2;
        }
        return run_set(setdir, inputs, ninputs, synth_streams, synth, level, bsize, channels, bps, verify);
    }
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-' && argv[i][1] >= '0' && argv[i][1] <= '9') level = atoi(argv[i] + 1);
        else if (!strcmp(argv[i], "-b") && i + 1 < argc) bsize = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--synth") && i + 1 < argc) synth = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--channels") && i + 1 < argc) channels = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--bps") && i + 1 < argc) bps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--verify")) verify = 1;
        else if (!in && !synth) in = argv[i];
        else out = argv[i];
    }
    if (!out || (!in && !synth)) {
        fprintf(stderr, "usage: %s [-0..-12] [-b blocksize] [--verify] (in.wav | --synth FRAMES [--channels C] [--bps B]) out.flac\n"
                        "       %s [-0..-12] [-b blocksize] --set OUTDIR [--verify] (in1.wav in2.wav ... | --synth-streams S --synth FRAMES [--channels C] [--bps B])\n",
                argv[0], argv[0]);
        fprintf(stderr, RECODE_USAGE, argv[0]);
        return 2;
    }
    wav_t w;
    memset(&w, 0, sizeof w);
    if (in) {
        if (wav_open(&w, in)) { fprintf(stderr, "cannot read %s as PCM WAV\n", in); return 1; }
        s.channels = w.channels; s.sample_rate = w.rate; s.bits_per_sample = w.bps; s.samples = w.frames;
    } else {
        s.channels = channels; s.sample_rate = 44100; s.bits_per_sample = bps;
    }
    s.params.compression = level;
    if (flake_amd_set_defaults(&s.params)) return 1;                 /* flake.c:528 */
    if (bsize > 0) s.params.block_size = bsize;
    if (synth) s.samples = (unsigned)synth * (unsigned)s.params.block_size;
    if (flake_amd_validate_params(&s) < 0) { fprintf(stderr, "invalid parameters\n"); return 1; }
    int hlen = flake_amd_encode_init(&s);                            /* flake.c:558 */
    if (hlen < 0) { fprintf(stderr, "encoder init failed (%d)\n", hlen); return 1; }
    if (verify && flake_amd_set_verify(&s, 1)) { fprintf(stderr, "cannot turn verification on\n"); return 1; }
    FILE *fo = fopen(out, "wb");
    if (!fo) { perror(out); return 1; }
    fwrite(s.header, 1, (size_t)hlen, fo);

    const int bs = s.params.block_size, nch = s.channels, batch = 256;
    int32_t *pcm = (int32_t *)malloc(sizeof(int32_t) * (size_t)batch * bs * nch);
    /* 16 bits per sample or fewer at a level without variable block size: the samples stay int16 all the way
     * (flake_amd_encode_frames_s16); everything else is widened to int32 as before -- also under the CPU comparison
     * modes FLAKE_AMD_HOST_ASSEMBLY=1 / FLAKE_AMD_HOST_VBS=1, which the int16 entry refuses */
    const char *eha = getenv("FLAKE_AMD_HOST_ASSEMBLY"), *ehv = getenv("FLAKE_AMD_HOST_VBS");
    const int cpu_mode = (eha && eha[0] == '1') || (ehv && ehv[0] == '1');
    const int narrow = s.bits_per_sample <= 16 && !s.params.variable_block_size && !cpu_mode;
    int16_t *pcm16 = narrow ? (int16_t *)malloc(sizeof(int16_t) * (size_t)batch * bs * nch) : NULL;
    if (!pcm || (narrow && !pcm16)) { fprintf(stderr, "out of memory\n"); return 1; }
    const size_t cap = (size_t)batch * bs * nch * 5 + 65536;
    uint8_t *buf = (uint8_t *)malloc(cap);
    uint64_t total_in = 0, total_out = (uint64_t)hlen;
    int64_t synth_left = synth, synth_pos = 0;
    for (;;) {
        uint32_t frames;
        if (synth) {
            int nb = synth_left < batch ? (int)synth_left : batch;
            if (nb <= 0) break;
            flake_amd_synth_pcm(pcm, synth_pos, nb, bs, nch, s.bits_per_sample);
            synth_pos += nb; synth_left -= nb;
            frames = (uint32_t)nb * (uint32_t)bs;
            if (narrow) for (size_t i = 0; i < (size_t)frames * nch; i++) pcm16[i] = (int16_t)pcm[i];
        } else {
            frames = wav_read(&w, pcm, pcm16, (uint32_t)batch * (uint32_t)bs);
            if (!frames) break;
        }
        const int nblocks = (int)(frames / (uint32_t)bs), tail = (int)(frames % (uint32_t)bs);
        long long n = narrow ? flake_amd_encode_frames_s16(&s, pcm16, nblocks, bs, tail, buf, cap, NULL)
                             : flake_amd_encode_frames(&s, pcm, nblocks, bs, tail, buf, cap, NULL);   /* flake.c:633 */
        if (n < 0) { fprintf(stderr, "encode error: %s\n", flake_amd_last_error(&s)); return 1; }
        fwrite(buf, 1, (size_t)n, fo);
        total_in += frames; total_out += (uint64_t)n;
        if (tail) break;
    }
    /* rewrite STREAMINFO with the final MD5 / max frame size (flake.c:668-679) */
    FlakeAmdStreaminfo si;
    uint8_t sib[34];
    if (!s.samples) s.samples = (unsigned)total_in;
    if (!flake_amd_get_streaminfo(&s, &si)) {
        si.samples = (unsigned)total_in;
        flake_amd_write_streaminfo(&si, sib);
        fseek(fo, 8, SEEK_SET);
        fwrite(sib, 1, 34, fo);
    }
    fclose(fo);
    fprintf(stderr, "%llu sample-frames -> %llu bytes (ratio %.3f)\n", (unsigned long long)total_in,
            (unsigned long long)total_out,
            total_in ? (double)total_out / ((double)total_in * nch * ((s.bits_per_sample + 7) / 8)) : 0.0);
    flake_amd_encode_close(&s);
    free(pcm); free(pcm16); free(buf);
    return 0;
}
