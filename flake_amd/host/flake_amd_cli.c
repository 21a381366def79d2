/*
 * flake_amd_cli.c -- minimal command-line harness on top of the host layer.  One mode per run; main() picks it from
 * the mode table at the end of the file and scans the switches that the mode accepts.  Every other word is a
 * positional argument.
 *
 *   flake_amd_cli [-0..-12] [-b blocksize] [--verify] in.wav out.flac
 *   flake_amd_cli [-0..-12] --synth FRAMES [--channels C] [--bps B] [--verify] out.flac
 *
 * run_encode: the block loop of the reference CLI (flake/flake.c:495-689: read a block of samples,
 * flake_encode_frame(), write the frame, rewrite STREAMINFO at the end), with the frames of many blocks encoded per GPU
 * batch.
 *
 *   flake_amd_cli [-0..-12] [-b blocksize] --set OUTDIR [--verify] in1.wav in2.wav ...
 *   flake_amd_cli [-0..-12] --set OUTDIR [--verify] --synth-streams S --synth FRAMES [--channels C] [--bps B]
 *
 * run_set encodes inputs of one format as a stream set (flake_amd_set_*): their blocks round-robin in shared GPU
 * batches, every stream's MD5 carried on the device, one OUTDIR/<name>.flac per input with its own STREAMINFO --
 * the file the single-input form writes for that input.
 *
 * --verify checks on the GPU that every frame decodes to its input (flake_amd_set_verify; for --set
 * flake_amd_set_enable_verify, every frame held to its own stream's numbering) and exits non-zero with the
 * verifier's message when one does not.
 *
 *   flake_amd_cli --decode in.flac out.wav
 *
 * run_decode turns a FLAC file back into canonical PCM WAV on the GPU (flake_amd_decode_*): it checks the "fLaC" marker,
 * reads STREAMINFO, skips the other metadata blocks (flac_load), finds the frames on the device (flake_amd_decode_index;
 * on the CPU, flake_amd_index_frames, with FLAKE_AMD_INDEX_HOST=1 or for a file of 2 GiB and more), decodes them in
 * batches and compares the MD5 of what it wrote with STREAMINFO's unless that is all zero (source_check).  A frame that
 * does not decode, or an MD5 mismatch, ends in a non-zero exit status with the frame named on stderr.
 *
 *   flake_amd_cli --decode --set OUTDIR a.flac b.flac ...
 *   flake_amd_cli --decode [--set OUTDIR] --skip N --until N ...
 *       a window of samples out of every file (sample counts, as flac's options of those names; --until is exclusive, 0 or
 *       absent: to the end): flake_amd_decode_set_windows on a set without MD5 -- the frames that overlap the window
 *       are found from the headers, indexing starts at the file's SEEKTABLE point at or before --skip where it has one
 *       (the whole file where that piece is refused), the WAV holds exactly the window and the MD5 is not checked.
 *
 * run_decode_set decodes files of one format (flac_set_load) through one decode set (flake_amd_decode_set_*): the
 * device finds every file's frames, one call per max_block_size among the files (flac_set_index; the CPU with
 * FLAKE_AMD_INDEX_HOST=1 or where the device cannot answer), the frames go round-robin into shared GPU batches
 * (pack_runs), every stream's MD5 is carried on the device and held against its STREAMINFO, and OUTDIR/<name>.wav is
 * written per input.  An input whose format differs from the first's is an error that names it.  A file that fails is
 * named on stderr and makes the exit status non-zero; the other files are still written in full.
 *
 *   flake_amd_cli [-0..-12] [-b blocksize] --recode --set OUTDIR [--verify] a.flac b.flac ...
 *
 * run_recode_set re-encodes FLAC files of one format at another level through one recode set (flake_amd_recode_set_*):
 * files loaded, frames found and packed as in --decode --set, decoded, re-cut into the new block size and encoded
 * without the samples leaving the device.  OUTDIR/<name>.flac is "fLaC" + the new STREAMINFO + frames, as the encoder
 * writes it; other metadata blocks are NOT carried over.  A file whose decode fails, or whose digest differs from a
 * non-zero source digest, is named on stderr, gets no output (one left by an earlier run is removed) and makes the exit
 * status non-zero; the other files are written.  --verify turns the recode set's on-device verification on.
 *
 *   flake_amd_cli ... --seekpoints N ...        (the single-file encode, --set and --recode --set)
 *
 * A seek point every N samples (flake_amd_seekpoints and its set forms; N at least 1): the file is "fLaC", STREAMINFO,
 * a SEEKTABLE block, then the header as without the switch (vendor comment, padding) and the frames.  The set modes
 * hold every file's frames until the end and write the exact table.  The single-file mode streams to disk: it reserves
 * ceil(samples / N) points (the total is the WAV's, or --synth's), and rewrites the table at the end, beside
 * STREAMINFO, the remainder filled with placeholder points.
 *
 *   flake_amd_cli --reseek N --set OUTDIR a.flac b.flac ...
 *
 * run_reseek adds or replaces the SEEKTABLE of existing files without decoding anything: files loaded and frames found
 * as in --decode --set (flac_set_load, flac_set_index), the points computed from the frames' headers
 * (flake_amd_seekpoints_of_frames), and OUTDIR/<name>.flac written as every metadata block of the source in order
 * except SEEKTABLE blocks, the new table right behind STREAMINFO, the frames byte for byte.  A file whose frames do not
 * cover it to the end is named on stderr, gets no output and makes the exit status non-zero; the others are written.
 *
 * Every mode leaves through one place that releases what it holds.  Only canonical PCM WAV (8/16/24/32 bit) is read;
 * this is a harness for the host API, not a replacement for the reference's libpcm_io.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flake_amd.h"

#define SET_USAGE "%s [-0..-12] [-b blocksize] --set OUTDIR [--verify] (in1.wav in2.wav ... | --synth-streams S --synth FRAMES [--channels C] [--bps B])\n"
#define RECODE_USAGE "usage: %s [-0..-12] [-b blocksize] --recode --set OUTDIR [--verify] a.flac b.flac ...\n" \
                     "       (files of one format; only STREAMINFO is written: other metadata blocks are not carried over)\n"
#define SEEK_USAGE "usage: %s ... --seekpoints N ...   (a seek point every N samples, N at least 1; with the single-file encode,\n" \
                   "       --set and --recode --set, not with --decode)\n" \
                   "       %s --reseek N --set OUTDIR a.flac b.flac ...   (a new SEEKTABLE for existing files)\n"
#define MAX_SEEK_POINTS 932067            /* what a metadata block's 24-bit length holds */

static uint32_t rd32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static void wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* what main() scanned: the switches of the active mode, and every other word in order */
typedef struct {
    int level, bsize, synth, synth_streams, channels, bps, verify;
    const char *setdir, *in, *out;
    int window;                      /* --skip or --until was given */
    unsigned long long skip, until;  /* samples; until 0: to the end */
    unsigned long long seekpoints;   /* --seekpoints N / --reseek N: a seek point every N samples; 0: none */
    char **pos;
    int npos;
} opts;

/* ---- PCM WAV in ------------------------------------------------------ */
typedef struct { FILE *f; int channels, rate, bps; uint32_t frames; } wav_t;

static int wav_parse(wav_t *w)
{
    uint8_t h[12], ck[8];
    if (fread(h, 1, 12, w->f) != 12 || memcmp(h, "RIFF", 4) || memcmp(h + 8, "WAVE", 4)) return -1;
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

static void wav_close(wav_t *w)
{
    if (w->f) fclose(w->f);
    w->f = NULL;
}

static int wav_open(wav_t *w, const char *path)
{
    w->f = fopen(path, "rb");
    if (w->f && !wav_parse(w)) return 0;
    fprintf(stderr, "cannot read %s as PCM WAV\n", path);
    wav_close(w);
    return -1;
}

/* up to `frames` sample-frames, sign-extended (pcm_io.c:155-277): interleaved int32 into dst, or -- dst16 given, files
 * of 16 bits per sample or fewer -- interleaved int16 into dst16 */
static uint32_t wav_read(wav_t *w, int32_t *dst, int16_t *dst16, uint32_t frames)
{
    const int bytes = (w->bps + 7) / 8;
    const size_t want = (size_t)frames * w->channels;
    uint8_t *raw = (uint8_t *)malloc(want * bytes + 1);
    size_t got = raw ? fread(raw, (size_t)bytes, want, w->f) : 0;
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

/* ---- PCM WAV out: 44 placeholder bytes, the samples, then the real header ---- */
static FILE *wav_begin(const char *path)
{
    static const uint8_t zero[44] = {0};
    FILE *f = fopen(path, "wb");
    if (f) fwrite(zero, 1, 44, f); else perror(path);
    return f;
}

/* `frames` sample-frames of si's format: int16 (16-bit streams: the 2-byte path all the way, little-endian hosts, as
 * the reader) or int32, repacked into raw[frames * channels * bytes per sample] */
static void wav_samples(FILE *f, const FlakeAmdStreaminfo *si, const void *pcm, size_t frames, uint8_t *raw)
{
    const size_t vals = frames * si->channels, wbytes = (si->bits_per_sample + 7) / 8;
    if (si->bits_per_sample == 16) {
        fwrite(pcm, 2, vals, f);
        return;
    }
    const int32_t *v = (const int32_t *)pcm;
    for (size_t i = 0; i < vals; i++) {
        const uint32_t u = wbytes == 1 ? (uint32_t)(v[i] + 128) : (uint32_t)v[i];
        for (size_t b = 0; b < wbytes; b++) raw[i * wbytes + b] = (uint8_t)(u >> (8 * b));
    }
    fwrite(raw, wbytes, vals, f);
}

static void wav_end(FILE *f, const FlakeAmdStreaminfo *si, unsigned long long frames)
{
    const int channels = (int)si->channels, bytes = ((int)si->bits_per_sample + 7) / 8;
    const uint32_t data = (uint32_t)frames * (uint32_t)(channels * bytes);
    uint8_t h[44];
    memcpy(h, "RIFF", 4); wr32(h + 4, 36 + data); memcpy(h + 8, "WAVEfmt ", 8); wr32(h + 16, 16);
    h[20] = 1; h[21] = 0; h[22] = (uint8_t)channels; h[23] = 0;
    wr32(h + 24, si->sample_rate); wr32(h + 28, si->sample_rate * (uint32_t)(channels * bytes));
    h[32] = (uint8_t)(channels * bytes); h[33] = 0; h[34] = (uint8_t)si->bits_per_sample; h[35] = 0;
    memcpy(h + 36, "data", 4); wr32(h + 40, data);
    fseek(f, 0, SEEK_SET);
    fwrite(h, 1, 44, f);
    fclose(f);
}

/* ---- the encoding side: parameters, the stream header, frames per stream ---- */
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

/* the frames of one call, back to back in buf: each to the output of its stream */
static int scatter(bytes_t *outs, const uint8_t *buf, const int *stream_of, const int *sizes, int count)
{
    for (int b = 0; b < count; b++) {
        if (bytes_add(&outs[stream_of[b]], buf, (size_t)sizes[b])) { fprintf(stderr, "out of memory\n"); return -1; }
        buf += sizes[b];
    }
    return 0;
}

/* a level's parameters (flake.c:528) for the format already in s, the block size overridden where one is given */
static int enc_params(FlakeAmdContext *s, const opts *o)
{
    s->params.compression = o->level;
    if (flake_amd_set_defaults(&s->params)) return -1;
    if (o->bsize > 0) s->params.block_size = o->bsize;
    if (flake_amd_validate_params(s) < 0) { fprintf(stderr, "invalid parameters\n"); return -1; }
    return 0;
}

/* the stream header of the single-input form (flake.c:558) for a set's files: STREAMINFO is rewritten per file */
static uint8_t *set_header(FlakeAmdContext *s, int *hlen)
{
    *hlen = flake_amd_encode_init(s);
    if (*hlen < 0) { fprintf(stderr, "encoder init failed (%d)\n", *hlen); return NULL; }
    uint8_t *header = (uint8_t *)malloc((size_t)*hlen);
    if (header) memcpy(header, s->header, (size_t)*hlen);
    flake_amd_encode_close(s);
    return header;
}

/* A whole SEEKTABLE metadata block, its 4-byte header (never the last block: `last` 0, or 1) and its content: n points
 * and `placeholders` placeholder points behind them.  malloc'd, *len bytes; NULL (with a word on stderr) where the
 * table is refused or memory is short */
static uint8_t *seektable_block(const FlakeAmdSeekPoint *pts, int n, long long placeholders, int last, size_t *len)
{
    const long long all = (long long)n + placeholders;
    uint8_t *b = all <= MAX_SEEK_POINTS ? (uint8_t *)malloc(4 + 18 * (size_t)all + 1) : NULL;
    if (!b || flake_amd_write_seektable(pts, n, (int)placeholders, b + 4, 18 * (size_t)all) != 18 * all) {
        fprintf(stderr, "cannot write a SEEKTABLE of %lld points (a block holds %d)\n", all, MAX_SEEK_POINTS);
        free(b);
        return NULL;
    }
    b[0] = (uint8_t)((last ? 0x80 : 0) | 3);
    b[1] = (uint8_t)((18 * all) >> 16); b[2] = (uint8_t)((18 * all) >> 8); b[3] = (uint8_t)(18 * all);
    *len = 4 + 18 * (size_t)all;
    return b;
}

/* the recorded points of one stream as its SEEKTABLE block: `get` is a set's getter, the exact table without placeholders */
typedef long long (*seek_getter)(const void *g, int stream, FlakeAmdSeekPoint *p, int cap);
static long long get_of_set(const void *g, int stream, FlakeAmdSeekPoint *p, int cap)
{
    return flake_amd_set_get_seekpoints((const FlakeAmdSet *)g, stream, p, cap);
}
static long long get_of_recode_set(const void *g, int stream, FlakeAmdSeekPoint *p, int cap)
{
    return flake_amd_recode_set_get_seekpoints((const FlakeAmdRecodeSet *)g, stream, p, cap);
}
static uint8_t *stream_seektable(seek_getter get, const void *g, int stream, size_t *len)
{
    const long long n = get(g, stream, NULL, 0);
    FlakeAmdSeekPoint *pts = n >= 0 && n <= MAX_SEEK_POINTS ? (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)(n ? n : 1)) : NULL;
    uint8_t *b = NULL;
    if (pts && get(g, stream, pts, (int)n) == n) b = seektable_block(pts, (int)n, 0, 0, len);
    else fprintf(stderr, "stream %d: its seek points cannot be read\n", stream);
    free(pts);
    return b;
}

/* one file of a set: the header with its own STREAMINFO (flake.c:668-679), then its frames; a SEEKTABLE block (seek,
 * or NULL for none) goes right behind STREAMINFO */
static int flac_write(const char *path, uint8_t *header, int hlen, const FlakeAmdStreaminfo *si, const uint8_t *seek,
                      size_t seek_len, const bytes_t *frames)
{
    FILE *fo = fopen(path, "wb");
    if (!fo) { perror(path); return -1; }
    flake_amd_write_streaminfo(si, header + 8);
    fwrite(header, 1, 42, fo);
    if (seek) fwrite(seek, 1, seek_len, fo);
    fwrite(header + 42, 1, (size_t)hlen - 42, fo);
    fwrite(frames->p, 1, frames->n, fo);
    fclose(fo);
    return 0;
}

/* ---- single file: WAV or the synthetic signal to FLAC ---------------- */
static int run_encode(const opts *o, const char *argv0)
{
    if (!o->out || (!o->in && !o->synth)) {
        fprintf(stderr, "usage: %s [-0..-12] [-b blocksize] [--verify] (in.wav | --synth FRAMES [--channels C] [--bps B]) out.flac\n"
                        "       " SET_USAGE, argv0, argv0);
        fprintf(stderr, RECODE_USAGE, argv0);
        return 2;
    }
    int rc = 1, open = 0;
    FlakeAmdContext s;
    wav_t w;
    FILE *fo = NULL;
    int32_t *pcm = NULL;
    int16_t *pcm16 = NULL;
    uint8_t *buf = NULL, *seek = NULL;
    memset(&s, 0, sizeof s);
    memset(&w, 0, sizeof w);
    if (o->in) {
        if (wav_open(&w, o->in)) goto out;
        s.channels = w.channels; s.sample_rate = w.rate; s.bits_per_sample = w.bps; s.samples = w.frames;
    } else {
        s.channels = o->channels; s.sample_rate = 44100; s.bits_per_sample = o->bps;
    }
    if (enc_params(&s, o)) goto out;
    if (o->synth) s.samples = (unsigned)o->synth * (unsigned)s.params.block_size;
    const int hlen = flake_amd_encode_init(&s);                      /* flake.c:558 */
    if (hlen < 0) { fprintf(stderr, "encoder init failed (%d)\n", hlen); goto out; }
    open = 1;
    if (o->verify && flake_amd_set_verify(&s, 1)) { fprintf(stderr, "cannot turn verification on\n"); goto out; }
    /* --seekpoints: the table is reserved now, ceil(samples / N) points -- no stream of that length has more -- and
     * rewritten at the end */
    long long reserved = 0;
    size_t seek_len = 0;
    if (o->seekpoints) {
        reserved = (long long)(((unsigned long long)s.samples + o->seekpoints - 1) / o->seekpoints);
        if (flake_amd_seekpoints(&s, o->seekpoints)) { fprintf(stderr, "cannot turn seek points on\n"); goto out; }
        seek = seektable_block(NULL, 0, reserved, 0, &seek_len);
        if (!seek) goto out;
    }
    fo = fopen(o->out, "wb");
    if (!fo) { perror(o->out); goto out; }
    fwrite(s.header, 1, 42, fo);                                     /* "fLaC" and STREAMINFO */
    if (seek) fwrite(seek, 1, seek_len, fo);
    fwrite(s.header + 42, 1, (size_t)hlen - 42, fo);

    const int bs = s.params.block_size, nch = s.channels, batch = 256;
    /* 16 bits per sample or fewer at a level without variable block size: the samples stay int16 all the way
     * (flake_amd_encode_frames_s16); everything else is widened to int32 as before -- also under the CPU comparison
     * modes FLAKE_AMD_HOST_ASSEMBLY=1 / FLAKE_AMD_HOST_VBS=1, which the int16 entry refuses */
    const char *eha = getenv("FLAKE_AMD_HOST_ASSEMBLY"), *ehv = getenv("FLAKE_AMD_HOST_VBS");
    const int cpu_mode = (eha && eha[0] == '1') || (ehv && ehv[0] == '1');
    const int narrow = s.bits_per_sample <= 16 && !s.params.variable_block_size && !cpu_mode;
    const size_t cap = (size_t)batch * bs * nch * 5 + 65536;
    pcm = (int32_t *)malloc(sizeof(int32_t) * (size_t)batch * bs * nch);
    pcm16 = narrow ? (int16_t *)malloc(sizeof(int16_t) * (size_t)batch * bs * nch) : NULL;
    buf = (uint8_t *)malloc(cap);
    if (!pcm || (narrow && !pcm16) || !buf) { fprintf(stderr, "out of memory\n"); goto out; }
    uint64_t total_in = 0, total_out = (uint64_t)hlen + seek_len;
    int64_t synth_left = o->synth, synth_pos = 0;
    for (;;) {
        uint32_t frames;
        if (o->synth) {
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
        if (n < 0) { fprintf(stderr, "encode error: %s\n", flake_amd_last_error(&s)); goto out; }
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
    if (seek) {
        /* the points that were recorded, as many as were reserved at the most, the remainder placeholders */
        const long long have = flake_amd_get_seekpoints(&s, NULL, 0);
        const long long take = have < reserved ? have : reserved;
        FlakeAmdSeekPoint *pts = take >= 0 ? (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)(take ? take : 1)) : NULL;
        size_t len = 0;
        uint8_t *table = pts && flake_amd_get_seekpoints(&s, pts, (int)take) == have
                             ? seektable_block(pts, (int)take, reserved - take, 0, &len) : NULL;
        free(pts);
        if (!table || len != seek_len) { fprintf(stderr, "the seek table could not be rewritten\n"); free(table); goto out; }
        fseek(fo, 42, SEEK_SET);
        fwrite(table, 1, len, fo);
        free(table);
    }
    fprintf(stderr, "%llu sample-frames -> %llu bytes (ratio %.3f)\n", (unsigned long long)total_in,
            (unsigned long long)total_out,
            total_in ? (double)total_out / ((double)total_in * nch * ((s.bits_per_sample + 7) / 8)) : 0.0);
    rc = 0;
out:
    if (fo) fclose(fo);
    if (open) flake_amd_encode_close(&s);
    wav_close(&w);
    free(pcm); free(pcm16); free(buf); free(seek);
    return rc;
}

/* ---- --set: many inputs of one format through one stream set -------- */
typedef struct {
    FlakeAmdSet *g;
    int sample_bytes, nch, cap_blocks, count;
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
    const int count = r->count;
    r->count = 0;
    return scatter(r->outs, r->buf, r->stream_of, r->sizes, count);
}

static int set_add(set_run *r, int stream, const char *block, int block_size)
{
    const size_t bytes = (size_t)block_size * r->nch * r->sample_bytes;
    memcpy(r->pcm + (size_t)r->count * bytes, block, bytes);
    r->stream_of[r->count++] = stream;
    return r->count == r->cap_blocks ? set_flush(r, block_size) : 0;
}

static int run_set(const opts *o, const char *argv0)
{
    const int ninputs = o->npos, synth = o->synth;
    if (!o->setdir || (!ninputs && (o->synth_streams < 1 || synth < 1)) || (ninputs && o->synth_streams)) {
        fprintf(stderr, "usage: " SET_USAGE, argv0);
        return 2;
    }
    const int S = ninputs ? ninputs : o->synth_streams;
    int rc = 1, hlen = 0;
    FlakeAmdContext s;
    set_run r;
    uint8_t *header = NULL;
    int *tail_of = NULL;
    memset(&s, 0, sizeof s);
    memset(&r, 0, sizeof r);
    wav_t *wavs = (wav_t *)calloc((size_t)S, sizeof(wav_t));
    uint32_t *frames = (uint32_t *)calloc((size_t)S, sizeof(uint32_t));
    char **data = (char **)calloc((size_t)S, sizeof(char *));
    bytes_t *outs = (bytes_t *)calloc((size_t)S, sizeof(bytes_t));
    if (!wavs || !frames || !data || !outs) { fprintf(stderr, "out of memory\n"); goto out; }
    for (int i = 0; i < ninputs; i++) {
        if (wav_open(&wavs[i], o->pos[i])) goto out;
        if (i && (wavs[i].channels != wavs[0].channels || wavs[i].rate != wavs[0].rate || wavs[i].bps != wavs[0].bps)) {
            fprintf(stderr, "%s: a set's inputs must share channels, sample rate and bits per sample\n", o->pos[i]);
            goto out;
        }
    }
    s.channels = ninputs ? wavs[0].channels : o->channels;
    s.sample_rate = ninputs ? wavs[0].rate : 44100;
    s.bits_per_sample = ninputs ? wavs[0].bps : o->bps;
    if (enc_params(&s, o)) goto out;
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
        if (!data[i] || ((!ninputs || !narrow) && !wide)) { fprintf(stderr, "out of memory\n"); free(wide); goto out; }
        if (ninputs) {
            frames[i] = wav_read(&wavs[i], wide, narrow ? (int16_t *)data[i] : NULL, frames[i]);
            wav_close(&wavs[i]);
        } else {
            /* stream i: the synthetic signal from frame index i * FRAMES on, so the streams differ */
            flake_amd_synth_pcm(wide, (int64_t)i * synth, synth, bs, nch, s.bits_per_sample);
        }
        if (wide && narrow) for (size_t k = 0; k < vals; k++) ((int16_t *)data[i])[k] = (int16_t)wide[k];
        else if (wide) memcpy(data[i], wide, (size_t)frames[i] * nch * sizeof(int32_t));
        free(wide);
    }
    header = set_header(&s, &hlen);
    if (!header) goto out;
    r.g = flake_amd_set_open(&s, S, s.params.variable_block_size ? FLAKE_AMD_SET_VBS : 0);
    if (!r.g) { fprintf(stderr, "%s\n", flake_amd_set_last_error(NULL)); goto out; }
    if (o->verify && flake_amd_set_enable_verify(r.g, 1)) { fprintf(stderr, "cannot turn verification on\n"); goto out; }
    if (o->seekpoints && flake_amd_set_seekpoints(r.g, o->seekpoints)) { fprintf(stderr, "cannot turn seek points on\n"); goto out; }
    r.sample_bytes = sample_bytes; r.nch = nch; r.cap_blocks = 1024; r.outs = outs;
    r.pcm = (char *)malloc((size_t)r.cap_blocks * bs * nch * sample_bytes);
    r.stream_of = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    r.sizes = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    r.buf_cap = (size_t)r.cap_blocks * bs * nch * 5 + 65536;
    r.buf = (uint8_t *)malloc(r.buf_cap);
    tail_of = (int *)malloc(sizeof(int) * (size_t)r.cap_blocks);
    if (!r.pcm || !r.stream_of || !r.sizes || !r.buf || !tail_of) { fprintf(stderr, "out of memory\n"); goto out; }
    const size_t bbytes = (size_t)bs * nch * sample_bytes;
    uint32_t rounds = 0;
    for (int i = 0; i < S; i++) if (frames[i] / (uint32_t)bs > rounds) rounds = frames[i] / (uint32_t)bs;
    for (uint32_t k = 0; k < rounds; k++)                       /* whole blocks, round-robin over the streams */
        for (int i = 0; i < S; i++)
            if (k < frames[i] / (uint32_t)bs && set_add(&r, i, data[i] + (size_t)k * bbytes, bs)) goto out;
    if (set_flush(&r, bs)) goto out;
    /* tails: every stream's last, short block in ONE ragged call (per cap_blocks streams), whatever their lengths */
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
            if (n < 0) { fprintf(stderr, "encode error: %s\n", flake_amd_set_last_error(r.g)); goto out; }
            if (scatter(outs, r.buf, r.stream_of, r.sizes, r.count)) goto out;
            r.count = 0;
        }
    }
    unsigned long long total_in = 0, total_out = 0;
    for (int i = 0; i < S; i++) {
        char path[4096];
        if (ninputs) {
            const char *base = strrchr(o->pos[i], '/');
            base = base ? base + 1 : o->pos[i];
            size_t len = strlen(base);
            if (len > 4 && !strcmp(base + len - 4, ".wav")) len -= 4;
            snprintf(path, sizeof path, "%s/%.*s.flac", o->setdir, (int)len, base);
        } else {
            snprintf(path, sizeof path, "%s/stream%05d.flac", o->setdir, i);
        }
        FlakeAmdStreaminfo si;
        if (flake_amd_set_get_streaminfo(r.g, i, &si)) { fprintf(stderr, "%s\n", flake_amd_set_last_error(r.g)); goto out; }
        size_t seek_len = 0;
        uint8_t *seek = o->seekpoints ? stream_seektable(get_of_set, r.g, i, &seek_len) : NULL;
        const int wrote = (o->seekpoints && !seek) ? -1 : flac_write(path, header, hlen, &si, seek, seek_len, &outs[i]);
        free(seek);
        if (wrote) goto out;
        total_in += frames[i]; total_out += (unsigned long long)hlen + seek_len + outs[i].n;
    }
    fprintf(stderr, "%d streams, %llu sample-frames -> %llu bytes (ratio %.3f)\n", S, total_in, total_out,
            total_in ? (double)total_out / ((double)total_in * nch * ((s.bits_per_sample + 7) / 8)) : 0.0);
    rc = 0;
out:
    if (r.g) flake_amd_set_close(r.g);
    for (int i = 0; i < S && wavs && data && outs; i++) { wav_close(&wavs[i]); free(data[i]); free(outs[i].p); }
    free(r.pcm); free(r.stream_of); free(r.sizes); free(r.buf); free(tail_of); free(header);
    free(wavs); free(frames); free(data); free(outs);
    return rc;
}

/* ---- FLAC in: a file whole in memory (a harness), its STREAMINFO, its frames ---- */
typedef struct {
    const char *path;
    uint8_t *file;
    size_t len, pos;                 /* the file, and where its next frame starts */
    const uint8_t *seek;             /* its SEEKTABLE block's content, where it has one */
    size_t seek_len;
    FlakeAmdStreaminfo si;
    int *sizes;                      /* every frame's size (flac_set_index, over the whole file) */
    size_t used;                     /* ... the bytes they cover */
    long long nframes, next;         /* ... how many, and the next one to hand over */
    int indexed;                     /* 1: a device call held it, 2: and answered */
    FILE *fo;
    unsigned long long total;
    int bad;                         /* named on stderr already */
    int skip;                        /* ... before it was a stream at all: it has no output file */
    int dead;                        /* its stream has failed in the set (the caller refreshes it for pack_runs) */
    char name[1024];                 /* OUTDIR/<name>.<ext> */
} flac_in;

static void flac_free(flac_in *fs, int n)
{
    for (int i = 0; i < n && fs; i++) {
        if (fs[i].fo) fclose(fs[i].fo);
        free(fs[i].file);
        free(fs[i].sizes);
    }
    free(fs);
}

static int flac_load(const char *path, flac_in *f)
{
    f->path = path;
    FILE *fi = fopen(path, "rb");
    if (!fi) { perror(path); return 1; }
    fseek(fi, 0, SEEK_END);
    const long flen = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    f->file = (uint8_t *)malloc(flen > 0 ? (size_t)flen : 1);
    const int got = f->file && flen >= 0 && fread(f->file, 1, (size_t)flen, fi) == (size_t)flen;
    fclose(fi);
    if (!got) { fprintf(stderr, "cannot read %s\n", path); return 1; }
    f->len = (size_t)flen;
    if (f->len < 4 + 4 + 34 || memcmp(f->file, "fLaC", 4) || (f->file[4] & 0x7F) != 0 ||
        ((size_t)f->file[5] << 16 | (size_t)f->file[6] << 8 | f->file[7]) != 34) {
        fprintf(stderr, "%s: not a FLAC file (no fLaC marker followed by STREAMINFO)\n", path);
        return 1;
    }
    if (flake_amd_read_streaminfo(f->file + 8, &f->si) < 0) { fprintf(stderr, "%s: invalid STREAMINFO\n", path); return 1; }
    size_t pos = 4;
    int last = 0;
    while (!last && pos + 4 <= f->len) {                                     /* skip every metadata block */
        last = f->file[pos] >> 7;
        const size_t blen = (size_t)f->file[pos + 1] << 16 | (size_t)f->file[pos + 2] << 8 | f->file[pos + 3];
        if ((f->file[pos] & 0x7F) == 3 && pos + 4 + blen <= f->len) { f->seek = f->file + pos + 4; f->seek_len = blen; }   /* (kept) */
        pos += 4 + blen;
    }
    if (!last || pos > f->len) { fprintf(stderr, "%s: metadata runs past the file\n", path); return 1; }
    f->pos = pos;
    return 0;
}

/* The prologue of a set of FLAC files.  A file that does not load is named (flac_load) and left out, like one that
 * fails later; the first one that loads sets the format, and `like` leaves as that format with the largest block size
 * among the files.  Every file gets its output name OUTDIR/<name>.<ext>.  -1 where the run cannot go on: a file of
 * another format, two files with one output name, or no file at all */
static int flac_set_load(flac_in *fs, char **inputs, int n, const char *outdir, const char *ext, const char *set_word,
                         FlakeAmdStreaminfo *like)
{
    int ref = -1;
    unsigned maxn = 16;
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (flac_load(inputs[i], f)) {
            f->bad = f->skip = 1;
            continue;
        }
        if (ref < 0) ref = i;
        if (f->si.channels != fs[ref].si.channels || f->si.bits_per_sample != fs[ref].si.bits_per_sample ||
            f->si.sample_rate != fs[ref].si.sample_rate) {
            fprintf(stderr, "%s: its format (%u channels, %u bits, %u Hz) differs from %s's: a %s set takes one format\n",
                    f->path, f->si.channels, f->si.bits_per_sample, f->si.sample_rate, fs[ref].path, set_word);
            return -1;
        }
        const unsigned mb = f->si.max_block_size ? f->si.max_block_size : 65535u;
        if (mb > maxn) maxn = mb;
        const char *base = strrchr(f->path, '/');
        base = base ? base + 1 : f->path;
        const char *dot = strrchr(base, '.');
        snprintf(f->name, sizeof f->name, "%s/%.*s.%s", outdir, (int)(dot ? dot - base : (long)strlen(base)), base, ext);
        for (int j = 0; j < i; j++)
            if (!fs[j].skip && !strcmp(fs[j].name, f->name)) {
                fprintf(stderr, "%s and %s would both be written to %s\n", fs[j].path, f->path, f->name);
                return -1;
            }
    }
    if (ref < 0) return -1;
    *like = fs[ref].si;
    like->max_block_size = maxn;
    return 0;
}

/* a set's exit status: 1 once any of its files has been named */
static int any_bad(const flac_in *fs, int n)
{
    int bad = 0;
    for (int i = 0; i < n; i++) bad |= fs[i].bad;
    return bad;
}

/* FLAKE_AMD_INDEX_HOST=1: frame discovery stays on the CPU (flake_amd_index_frames) */
static int index_on_host(void)
{
    const char *e = getenv("FLAKE_AMD_INDEX_HOST");
    return e && *e && strcmp(e, "0");
}

/* The frames of every loaded file.  On the device (K8) through ix, any decode set's handle: one call per
 * max_block_size among the files (a call holds one format; as a rule, one call), their frame bytes as ranges of one
 * buffer, while a call stays below 2 GiB.  Without ix, where the device cannot answer, or for what is left over, on the
 * CPU file by file.  A file whose frames end early is named, in file order after all indexing, and keeps the frames up
 * to there */
static void flac_set_index(flac_in *fs, int n, FlakeAmdDecodeSet *ix)
{
    int *member = (int *)malloc(sizeof(int) * (size_t)n);
    size_t *first = (size_t *)malloc(sizeof(size_t) * ((size_t)n + 1)), *cons = (size_t *)malloc(sizeof(size_t) * (size_t)n);
    long long *frames = (long long *)malloc(sizeof(long long) * (size_t)n);
    for (int i = 0; i < n; i++)
        if (!fs[i].skip) fs[i].sizes = (int *)malloc(sizeof(int) * ((fs[i].len - fs[i].pos) / 8 + 2));
    for (int lead = 0; lead < n && ix && member && first && cons && frames; lead++) {
        if (fs[lead].skip || fs[lead].indexed) continue;
        const unsigned mbs = fs[lead].si.max_block_size;
        size_t tot = 0;
        int members = 0;
        for (int i = lead; i < n; i++) {
            flac_in *f = &fs[i];
            const size_t left = f->len - f->pos;
            if (f->skip || f->indexed || !f->sizes || f->si.max_block_size != mbs || tot + left >= ((size_t)1 << 31)) continue;
            f->indexed = 1;
            member[members] = i;
            first[members++] = tot;
            tot += left;
        }
        first[members] = tot;
        const int cap = (int)(tot / 8) + members + 1;
        uint8_t *cat = (uint8_t *)malloc(tot + 1);         /* the members' frames, one range each */
        int *sizes = (int *)malloc(sizeof(int) * (size_t)cap);
        for (int r = 0; r < members && cat; r++) {
            const flac_in *f = &fs[member[r]];
            memcpy(cat + first[r], f->file + f->pos, f->len - f->pos);
        }
        if (members && cat && sizes &&
            flake_amd_decode_set_index(ix, mbs, cat, first, members, sizes, cap, frames, cons) == 0) {
            const int *mine = sizes;                    /* the ranges' sizes back to back; a refused range has none */
            for (int r = 0; r < members; r++) {
                flac_in *f = &fs[member[r]];
                f->indexed = 2;
                f->nframes = frames[r];
                f->used = cons[r];
                if (frames[r] > 0) memcpy(f->sizes, mine, sizeof(int) * (size_t)frames[r]);
                if (frames[r] > 0) mine += frames[r];
            }
        }
        free(cat); free(sizes);
    }
    free(member); free(first); free(cons); free(frames);
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip) continue;
        const size_t left = f->len - f->pos;
        if (f->indexed != 2)
            f->nframes = f->sizes ? flake_amd_index_frames(&f->si, f->file + f->pos, left, f->sizes, (int)(left / 8 + 2), &f->used) : -1;
        if (f->nframes < 0 || f->used != left) {
            fprintf(stderr, "%s: frame %lld (at byte %llu): %s\n", f->path, f->nframes < 0 ? 0ll : f->nframes,
                    (unsigned long long)(f->pos + f->used),
                    f->nframes < 0 ? "not a frame header of this stream" : "the frame is cut or its CRC-16 fails");
            f->bad = 1;
            if (f->nframes < 0) f->nframes = 0;
        }
    }
}

/* ---- the round-robin packer: a call takes up to `per` frames of every file that has some left ---- */
typedef struct {
    int per;
    int *sor, *fof, *csz;            /* per run: its stream and its frames; per frame: its size */
    uint8_t *bytes;                  /* the frames back to back */
    size_t cap;
    int nruns, nframes;              /* what the last pack_runs made */
    size_t nbytes;
} run_pack;

static int pack_open(run_pack *p, int n, unsigned maxn)
{
    p->per = (int)((4u << 20) / maxn / (unsigned)n);
    if (p->per > 64) p->per = 64;
    if (p->per < 1) p->per = 1;
    p->sor = (int *)malloc(sizeof(int) * (size_t)n);
    p->fof = (int *)malloc(sizeof(int) * (size_t)n);
    p->csz = (int *)malloc(sizeof(int) * (size_t)n * (size_t)p->per);
    return p->sor && p->fof && p->csz ? 0 : -1;
}

static void pack_free(run_pack *p) { free(p->sor); free(p->fof); free(p->csz); free(p->bytes); }

/* one run per file that is loaded, has frames left and whose stream is not dead: the number of runs (0: no file has
 * frames left), -1 out of memory */
static int pack_runs(run_pack *p, flac_in *fs, int n)
{
    p->nruns = p->nframes = 0;
    p->nbytes = 0;
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip || f->dead || f->next >= f->nframes) continue;
        const int take = f->nframes - f->next < p->per ? (int)(f->nframes - f->next) : p->per;
        size_t rb = 0;
        for (int k = 0; k < take; k++) { p->csz[p->nframes++] = f->sizes[f->next + k]; rb += (size_t)f->sizes[f->next + k]; }
        if (p->nbytes + rb > p->cap) {
            uint8_t *more = (uint8_t *)realloc(p->bytes, (p->nbytes + rb) * 2);
            if (!more) return -1;
            p->bytes = more;
            p->cap = (p->nbytes + rb) * 2;
        }
        memcpy(p->bytes + p->nbytes, f->file + f->pos, rb);
        p->nbytes += rb;
        f->pos += rb;
        f->next += take;
        p->sor[p->nruns] = i;
        p->fof[p->nruns++] = take;
    }
    return p->nruns;
}

/* Is what was decoded what the source's STREAMINFO announces: its MD5 unless that is all zero, its sample count unless
 * that is 0.  `samples` is held to the 32 bits that the CLI's STREAMINFO carries: the decoders pass their running count,
 * --recode the new STREAMINFO's 32-bit count, for which neither the mask nor the wider print changes anything.
 * 1 with the file named, 0 where it matches */
static int source_check(const char *path, const FlakeAmdStreaminfo *src, const uint8_t md5[16], unsigned long long samples)
{
    static const uint8_t zero[16] = {0};
    if (memcmp(src->md5sum, zero, 16) && memcmp(src->md5sum, md5, 16)) {
        fprintf(stderr, "%s: MD5 mismatch: the decoded samples are not what STREAMINFO's signature was made of\n", path);
        return 1;
    }
    if (src->samples && (unsigned long long)src->samples != (samples & 0xFFFFFFFFull)) {
        fprintf(stderr, "%s: %llu samples decoded, STREAMINFO says %u\n", path, samples, src->samples);
        return 1;
    }
    return 0;
}

/* ---- --decode: a FLAC file back to canonical PCM WAV ----------------- */
static int run_decode(const char *in, const char *out)
{
    int rc = 1;
    flac_in f;
    FlakeAmdDecoder *d = NULL;
    FILE *fo = NULL;
    int *sizes = NULL, *all = NULL;
    void *pcm = NULL;
    uint8_t *raw = NULL;
    unsigned long long total = 0, nframes_done = 0;
    memset(&f, 0, sizeof f);
    if (flac_load(in, &f)) goto out;
    const FlakeAmdStreaminfo *si = &f.si;
    d = flake_amd_decode_open(si);
    if (!d) { fprintf(stderr, "decoder init failed: %s\n", flake_amd_decode_last_error(NULL)); goto out; }
    fo = wav_begin(out);
    if (!fo) goto out;
    const int narrow = si->bits_per_sample == 16;                            /* int16 all the way (the 2-byte path) */
    const int maxn = si->max_block_size ? (int)si->max_block_size : 65535;
    const int batch = (4 << 20) / maxn < 1024 ? (4 << 20) / maxn : 1024;     /* frames per round: about 4M samples */
    const size_t cap = (size_t)batch * (size_t)maxn;
    sizes = (int *)malloc(sizeof(int) * (size_t)batch);
    pcm = malloc(cap * si->channels * (narrow ? 2 : 4));
    raw = (uint8_t *)malloc(cap * si->channels * ((si->bits_per_sample + 7) / 8));
    if (!sizes || !pcm || !raw) { fprintf(stderr, "out of memory\n"); goto out; }
    /* the frames of the whole file, found on the device in one call (K8): the same frames as the CPU finds piece by
     * piece below, since a piece's last frame ends at the header the next piece begins with.  FLAKE_AMD_INDEX_HOST=1,
     * or a file the device indexer refuses (2 GiB and more), keeps the CPU */
    long long all_n = 0, all_next = 0;
    int on_device = 0;
    if (!index_on_host() && f.pos < f.len && f.len - f.pos < ((size_t)1 << 31)) {
        const int all_cap = (int)((f.len - f.pos) / 8 + 1);
        size_t all_used = 0;
        all = (int *)malloc(sizeof(int) * (size_t)all_cap);
        all_n = all ? flake_amd_decode_index(d, f.file + f.pos, f.len - f.pos, all, all_cap, &all_used) : -2;
        on_device = all_n != -2;
    }
    rc = 0;
    while (f.pos < f.len) {
        size_t used = 0;
        long long nf;
        if (on_device) {
            nf = all_n < 0 ? -1 : (all_n - all_next < batch ? all_n - all_next : batch);
            for (long long k = 0; k < nf; k++) { sizes[k] = all[all_next + k]; used += (size_t)sizes[k]; }
            if (nf > 0) all_next += nf;
        } else {
            nf = flake_amd_index_frames(si, f.file + f.pos, f.len - f.pos, sizes, batch, &used);
        }
        if (nf <= 0) {
            fprintf(stderr, "%s: frame %llu (at byte %llu, after %llu samples): %s\n", in, nframes_done,
                    (unsigned long long)f.pos, total,
                    nf < 0 ? "not a frame header of this stream" : "the frame is cut or its CRC-16 fails");
            rc = 1;
            break;
        }
        const long long ns = flake_amd_decode_frames(d, f.file + f.pos, used, sizes, (int)nf, pcm, narrow ? 2 : 4, cap);
        if (ns < 0) { fprintf(stderr, "decode error: %s\n", flake_amd_decode_last_error(d)); rc = 1; break; }
        wav_samples(fo, si, pcm, (size_t)ns, raw);
        total += (unsigned long long)ns;
        nframes_done += (unsigned long long)nf;
        f.pos += used;
    }
    if (!rc) {
        uint8_t md5[16];
        flake_amd_decode_md5(d, md5);
        rc = source_check(in, si, md5, total);
    }
    if (!rc) fprintf(stderr, "%llu sample-frames decoded\n", total);
out:
    if (fo) wav_end(fo, &f.si, total);
    if (d) flake_amd_decode_close(d);
    free(f.file); free(sizes); free(pcm); free(raw); free(all);
    return rc;
}

/* ---- --decode --set: many FLAC files of one format through one decode set ---- */
static int run_decode_set(const opts *o)
{
    const int n = o->npos;
    if (n < 1) { fprintf(stderr, "--decode --set needs input files\n"); return 2; }
    int rc = 1;
    FlakeAmdStreaminfo like;
    FlakeAmdDecodeSet *g = NULL;
    run_pack p;
    long long *rs = NULL, *ro = NULL;
    void *pcm = NULL;
    uint8_t *raw = NULL;
    memset(&p, 0, sizeof p);
    flac_in *fs = (flac_in *)calloc((size_t)n, sizeof *fs);
    if (!fs || flac_set_load(fs, o->pos, n, o->setdir, "wav", "decode", &like)) goto out;
    const size_t nch = like.channels, maxn = like.max_block_size;
    const int narrow = like.bits_per_sample == 16;
    g = flake_amd_decode_set_open(&like, n, 0);
    if (!g) { fprintf(stderr, "decode set init failed: %s\n", flake_amd_decode_set_last_error(NULL)); goto out; }
    flac_set_index(fs, n, index_on_host() ? NULL : g);
    for (int i = 0; i < n; i++)
        if (!fs[i].skip && !(fs[i].fo = wav_begin(fs[i].name))) goto out;
    if (pack_open(&p, n, like.max_block_size)) { fprintf(stderr, "out of memory\n"); goto out; }
    const size_t cap = (size_t)n * (size_t)p.per * maxn;
    rs = (long long *)malloc(sizeof(long long) * (size_t)n);
    ro = (long long *)malloc(sizeof(long long) * (size_t)n);
    pcm = malloc(cap * nch * (narrow ? 2 : 4));
    raw = (uint8_t *)malloc((size_t)p.per * maxn * nch * ((like.bits_per_sample + 7) / 8));
    if (!rs || !ro || !pcm || !raw) { fprintf(stderr, "out of memory\n"); goto out; }
    for (;;) {
        for (int i = 0; i < n; i++) fs[i].dead = flake_amd_decode_set_failed(g, i, NULL, NULL) == 1;
        const int nruns = pack_runs(&p, fs, n);
        if (nruns < 0) { fprintf(stderr, "out of memory\n"); goto out; }
        if (!nruns) break;
        if (flake_amd_decode_set_frames(g, nruns, p.sor, p.fof, p.bytes, p.nbytes, p.csz, pcm, narrow ? 2 : 4, cap, rs) < 0 ||
            flake_amd_decode_set_run_offsets(g, ro, nruns) != nruns) {
            fprintf(stderr, "decode error: %s\n", flake_amd_decode_set_last_error(g));
            goto out;
        }
        for (int r = 0; r < nruns; r++) {
            flac_in *f = &fs[p.sor[r]];
            if (rs[r] < 0) {
                long long fr = -1;
                int st = 0;
                flake_amd_decode_set_failed(g, p.sor[r], &fr, &st);
                fprintf(stderr, "%s: frame %lld does not decode (status %d)\n", f->path, fr, st);
                f->bad = 1;
                continue;
            }
            wav_samples(f->fo, &like, (const char *)pcm + (size_t)ro[r] * nch * (narrow ? 2 : 4), (size_t)rs[r], raw);
            f->total += (unsigned long long)rs[r];
        }
    }
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip) continue;
        uint8_t md5[16];
        wav_end(f->fo, &like, f->total);
        f->fo = NULL;
        if (!f->bad && flake_amd_decode_set_md5(g, i, md5) != 0) {
            fprintf(stderr, "%s: %s\n", f->path, flake_amd_decode_set_last_error(g));
            f->bad = 1;
        } else if (!f->bad) {
            f->bad = source_check(f->path, &f->si, md5, f->total);
        }
        if (!f->bad) fprintf(stderr, "%s: %llu sample-frames decoded\n", f->path, f->total);
    }
    fprintf(stderr, "%lld device batches\n", flake_amd_decode_set_device_batches(g));
    rc = any_bad(fs, n);
out:
    if (g) flake_amd_decode_set_close(g);
    pack_free(&p);
    free(rs); free(ro); free(pcm); free(raw);
    flac_free(fs, n);
    return rc;
}

/* ---- --recode --set: many FLAC files of one format re-encoded through one recode set ---- */
static int run_recode_set(const opts *o, const char *argv0)
{
    const int n = o->npos;
    if (!o->setdir || !n) { fprintf(stderr, RECODE_USAGE, argv0); return 2; }
    int rc = 1, hlen = 0, bcap = 0;
    FlakeAmdStreaminfo like;
    FlakeAmdContext s;
    FlakeAmdRecodeSet *g = NULL;
    run_pack p;
    int *bstream = NULL, *bbytes = NULL;
    uint8_t *obuf = NULL, *header = NULL;
    size_t obuf_cap = 0;
    memset(&s, 0, sizeof s);
    memset(&p, 0, sizeof p);
    flac_in *fs = (flac_in *)calloc((size_t)n, sizeof *fs);
    bytes_t *outs = (bytes_t *)calloc((size_t)n, sizeof *outs);
    if (!fs || !outs || flac_set_load(fs, o->pos, n, o->setdir, "flac", "recode", &like)) goto out;
    /* the encoder's parameters, and the stream header of the single-input form with STREAMINFO rewritten per file */
    s.channels = (int)like.channels; s.sample_rate = (int)like.sample_rate; s.bits_per_sample = (int)like.bits_per_sample;
    if (enc_params(&s, o)) goto out;
    header = set_header(&s, &hlen);
    if (!header) goto out;
    /* the frames of every file, found through a throwaway decode set's handle */
    FlakeAmdDecodeSet *ix = index_on_host() ? NULL : flake_amd_decode_set_open(&like, 1, FLAKE_AMD_SET_MD5_OFF);
    flac_set_index(fs, n, ix);
    if (ix) flake_amd_decode_set_close(ix);
    g = flake_amd_recode_set_open(&like, &s, n, s.params.variable_block_size ? FLAKE_AMD_SET_VBS : 0);
    if (!g) { fprintf(stderr, "recode set init failed: %s\n", flake_amd_recode_set_last_error(NULL)); goto out; }
    if (o->verify && flake_amd_recode_set_enable_verify(g, 1)) { fprintf(stderr, "cannot turn verification on\n"); goto out; }
    if (o->seekpoints && flake_amd_recode_set_seekpoints(g, o->seekpoints)) { fprintf(stderr, "cannot turn seek points on\n"); goto out; }
    if (pack_open(&p, n, like.max_block_size)) { fprintf(stderr, "out of memory\n"); goto out; }
    for (int last = 0; !last;) {
        int nb = 0;
        for (int i = 0; i < n; i++) fs[i].dead = flake_amd_recode_set_failed(g, i, NULL, NULL) == 1;
        const int nruns = pack_runs(&p, fs, n);
        if (nruns < 0) { fprintf(stderr, "out of memory\n"); goto out; }
        last = !nruns;                     /* no frames left: the tails */
        size_t need = 0;
        long long need_blocks = 0;
        flake_amd_recode_set_out_bound(g, last ? -1 : p.nframes, &need, &need_blocks);
        if (need > obuf_cap || need_blocks > bcap) {
            free(obuf); free(bstream); free(bbytes);
            obuf_cap = need + 65536;
            bcap = (int)need_blocks + 1024;
            obuf = (uint8_t *)malloc(obuf_cap);
            bstream = (int *)malloc(sizeof(int) * (size_t)bcap);
            bbytes = (int *)malloc(sizeof(int) * (size_t)bcap);
            if (!obuf || !bstream || !bbytes) { fprintf(stderr, "out of memory\n"); goto out; }
        }
        const long long w = last ? flake_amd_recode_set_finish(g, obuf, obuf_cap, bstream, bbytes, bcap, &nb)
                                 : flake_amd_recode_set_frames(g, nruns, p.sor, p.fof, p.bytes, p.nbytes, p.csz, obuf, obuf_cap,
                                                               bstream, bbytes, bcap, &nb);
        if (w < 0) { fprintf(stderr, "recode error: %s\n", flake_amd_recode_set_last_error(g)); goto out; }
        if (scatter(outs, obuf, bstream, bbytes, nb)) goto out;
    }
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip) continue;
        long long fr = -1;
        int st = 0;
        FlakeAmdStreaminfo si;
        memset(&si, 0, sizeof si);
        if (flake_amd_recode_set_failed(g, i, &fr, &st) == 1) {
            fprintf(stderr, "%s: frame %lld does not decode (status %d)\n", f->path, fr, st);
            f->bad = 1;
        } else if (!f->bad && flake_amd_recode_set_get_streaminfo(g, i, &si)) {
            fprintf(stderr, "%s: %s\n", f->path, flake_amd_recode_set_last_error(g));
            f->bad = 1;
        } else if (!f->bad) {
            f->bad = source_check(f->path, &f->si, si.md5sum, si.samples);
        }
        /* a file named above gets no output, and one from an earlier run does not stay in its place */
        size_t seek_len = 0;
        uint8_t *seek = (!f->bad && o->seekpoints) ? stream_seektable(get_of_recode_set, g, i, &seek_len) : NULL;
        if (!f->bad && o->seekpoints && !seek) f->bad = 1;
        if (f->bad) remove(f->name);
        else if (flac_write(f->name, header, hlen, &si, seek, seek_len, &outs[i])) f->bad = 1;
        else fprintf(stderr, "%s: %u sample-frames -> %llu bytes\n", f->path, si.samples, (unsigned long long)hlen + seek_len + outs[i].n);
        free(seek);
    }
    long long db = 0, eb = 0;
    flake_amd_recode_set_device_batches(g, &db, &eb);
    fprintf(stderr, "%lld decode batches, %lld encode batches\n", db, eb);
    rc = any_bad(fs, n);
out:
    if (g) flake_amd_recode_set_close(g);
    for (int i = 0; i < n && outs; i++) free(outs[i].p);
    pack_free(&p);
    free(outs); free(bstream); free(bbytes); free(obuf); free(header);
    flac_free(fs, n);
    return rc;
}

/* ---- --reseek N --set: a new SEEKTABLE for existing files, nothing decoded ---- */

/* f as OUTDIR/<name>.flac with the table `seek` (a whole metadata block): STREAMINFO, the table, every other metadata
 * block of the source in order except its SEEKTABLE blocks, the last of them all flagged as such, then the frames */
static int reseek_write(const flac_in *f, uint8_t *seek, size_t seek_len)
{
    FILE *fo = fopen(f->name, "wb");
    if (!fo) { perror(f->name); return -1; }
    int kept = 0;                          /* the source's blocks behind STREAMINFO that stay (flac_load has walked them) */
    for (size_t pos = 4 + 4 + 34; pos < f->pos; pos += 4 + ((size_t)f->file[pos + 1] << 16 | (size_t)f->file[pos + 2] << 8 | f->file[pos + 3]))
        kept += (f->file[pos] & 0x7F) != 3;
    fwrite(f->file, 1, 4, fo);
    fputc(0, fo);                          /* STREAMINFO, not the last block: the table follows */
    fwrite(f->file + 5, 1, 3 + 34, fo);
    seek[0] = (uint8_t)((kept ? 0 : 0x80) | 3);
    fwrite(seek, 1, seek_len, fo);
    for (size_t pos = 4 + 4 + 34; pos < f->pos;) {
        const size_t blen = (size_t)f->file[pos + 1] << 16 | (size_t)f->file[pos + 2] << 8 | f->file[pos + 3];
        if ((f->file[pos] & 0x7F) != 3) {
            fputc((f->file[pos] & 0x7F) | (--kept ? 0 : 0x80), fo);
            fwrite(f->file + pos + 1, 1, 3 + blen, fo);
        }
        pos += 4 + blen;
    }
    fwrite(f->file + f->pos, 1, f->len - f->pos, fo);
    const int bad = ferror(fo);
    fclose(fo);
    if (bad) fprintf(stderr, "%s: write error\n", f->name);
    return bad ? -1 : 0;
}

static int run_reseek(const opts *o, const char *argv0)
{
    const int n = o->npos;
    if (!o->setdir || !n || !o->seekpoints) { fprintf(stderr, SEEK_USAGE, argv0, argv0); return 2; }
    int rc = 1;
    FlakeAmdStreaminfo like;
    flac_in *fs = (flac_in *)calloc((size_t)n, sizeof *fs);
    if (!fs || flac_set_load(fs, o->pos, n, o->setdir, "flac", "reseek", &like)) goto out;
    /* the frames of every file, found through a throwaway decode set's handle */
    FlakeAmdDecodeSet *ix = index_on_host() ? NULL : flake_amd_decode_set_open(&like, 1, FLAKE_AMD_SET_MD5_OFF);
    flac_set_index(fs, n, ix);
    if (ix) flake_amd_decode_set_close(ix);
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip || f->bad) continue;   /* named already: it did not load, or its frames do not cover it to the end */
        const uint8_t *frames = f->file + f->pos;
        const long long np = flake_amd_seekpoints_of_frames(&f->si, frames, f->used, f->sizes, (int)f->nframes, o->seekpoints, NULL, 0);
        FlakeAmdSeekPoint *pts = np >= 0 && np <= MAX_SEEK_POINTS ? (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)(np ? np : 1)) : NULL;
        size_t seek_len = 0;
        uint8_t *seek = NULL;
        if (pts && flake_amd_seekpoints_of_frames(&f->si, frames, f->used, f->sizes, (int)f->nframes, o->seekpoints, pts, (int)np) == np)
            seek = seektable_block(pts, (int)np, 0, 0, &seek_len);
        if (!seek) fprintf(stderr, "%s: no seek table could be made of its %lld frames\n", f->path, f->nframes);
        if (!seek || reseek_write(f, seek, seek_len)) f->bad = 1;
        else fprintf(stderr, "%s: %lld seek points over %lld frames\n", f->path, np, f->nframes);
        free(pts); free(seek);
    }
    rc = any_bad(fs, n);
out:
    flac_free(fs, n);
    return rc;
}

/* ---- --decode --skip N --until N: a window of samples out of every file ---- */

/* The frames the window needs, by the file's SEEKTABLE: the piece from the last seek point at or before `skip` to the first
 * one at or behind `until` is indexed on its own.  0 with f->pos, f->sizes, f->nframes describing the piece; -1 where the
 * file has no usable table or the piece is refused (a point that lies inside a frame): the whole file is indexed then */
static int seek_piece(flac_in *f, unsigned long long skip, unsigned long long until)
{
    if (!f->seek || !f->seek_len) return -1;
    const long long np = flake_amd_read_seektable(f->seek, f->seek_len, NULL, 0);
    if (np < 1) return -1;
    FlakeAmdSeekPoint *pts = (FlakeAmdSeekPoint *)malloc(sizeof *pts * (size_t)np);
    int rc = -1;
    if (pts && flake_amd_read_seektable(f->seek, f->seek_len, pts, (int)np) == np) {
        const long long a = flake_amd_seek_lookup(pts, (int)np, skip);
        long long b = until ? flake_amd_seek_lookup(pts, (int)np, until - 1) + 1 : np;     /* the first point at or behind until */
        const size_t left = f->len - f->pos;
        const size_t from = a < 0 ? 0 : (size_t)pts[a].offset, to = b < np ? (size_t)pts[b].offset : left;
        if ((a < 0 || pts[a].offset < left) && (b >= np || pts[b].offset <= left) && from < to) {
            const int cap = (int)((to - from) / 8 + 2);
            int *sizes = (int *)malloc(sizeof(int) * (size_t)cap);
            size_t used = 0;
            const long long nf = sizes ? flake_amd_index_frames(&f->si, f->file + f->pos + from, to - from, sizes, cap, &used) : -1;
            if (nf > 0 && used == to - from) {
                f->pos += from;
                f->sizes = sizes;
                f->nframes = nf;
                f->used = used;
                rc = 0;
            } else {
                free(sizes);
            }
        }
    }
    free(pts);
    return rc;
}

static int run_decode_windows(const opts *o)
{
    const int single = !o->setdir, n = single ? 1 : o->npos;
    if (n < 1) { fprintf(stderr, "--decode --set needs input files\n"); return 2; }
    int rc = 1;
    FlakeAmdStreaminfo like;
    FlakeAmdDecodeSet *g = NULL;
    int *fow = NULL, *sizes = NULL, *status = NULL, *pieced = NULL;
    unsigned *fixed = NULL;
    unsigned long long *first = NULL;
    long long *count = NULL, *got = NULL;
    uint8_t *bytes = NULL, *raw = NULL;
    void *pcm = NULL;
    flac_in *fs = (flac_in *)calloc((size_t)n, sizeof *fs);
    if (!fs) goto out;
    if (single) {
        if (flac_load(o->pos[0], &fs[0])) goto out;
        snprintf(fs[0].name, sizeof fs[0].name, "%s", o->pos[1]);
        like = fs[0].si;
        if (!like.max_block_size || like.max_block_size < 16) like.max_block_size = like.max_block_size ? 16 : 65535u;
    } else if (flac_set_load(fs, o->pos, n, o->setdir, "wav", "decode", &like)) {
        goto out;
    }
    fprintf(stderr, "--skip / --until: the MD5 of the decoded samples is not checked\n");
    const size_t nch = like.channels;
    const int narrow = like.bits_per_sample == 16;
    g = flake_amd_decode_set_open(&like, n, FLAKE_AMD_SET_MD5_OFF);
    if (!g) { fprintf(stderr, "decode set init failed: %s\n", flake_amd_decode_set_last_error(NULL)); goto out; }
    /* the frames: a piece between two seek points where the file's SEEKTABLE gives one, else the whole file */
    pieced = (int *)calloc((size_t)n, sizeof(int));
    if (!pieced) { fprintf(stderr, "out of memory\n"); goto out; }
    for (int i = 0; i < n; i++)
        if (!fs[i].skip && seek_piece(&fs[i], o->skip, o->until) == 0) pieced[i] = fs[i].skip = 1;    /* (hidden from the indexer) */
    flac_set_index(fs, n, index_on_host() ? NULL : g);
    for (int i = 0; i < n; i++)
        if (pieced[i]) fs[i].skip = 0;
    /* one window per file, all in one call */
    fow = (int *)calloc((size_t)n, sizeof(int));
    fixed = (unsigned *)calloc((size_t)n, sizeof(unsigned));
    first = (unsigned long long *)calloc((size_t)n, sizeof *first);
    count = (long long *)calloc((size_t)n, sizeof *count);
    got = (long long *)calloc((size_t)n, sizeof *got);
    status = (int *)calloc((size_t)n, sizeof(int));
    if (!fow || !fixed || !first || !count || !got || !status) { fprintf(stderr, "out of memory\n"); goto out; }
    size_t nbytes = 0, cap = 0;
    long long nframes = 0, most = 0;
    for (int i = 0; i < n; i++) {
        const flac_in *f = &fs[i];
        if (f->skip || f->nframes <= 0) continue;
        const unsigned maxn = f->si.max_block_size ? f->si.max_block_size : 65535u;
        const long long room = f->nframes * (long long)maxn;          /* no run delivers more */
        fow[i] = (int)f->nframes;
        fixed[i] = f->si.min_block_size == f->si.max_block_size ? f->si.max_block_size : 0;
        first[i] = o->skip;
        count[i] = o->until ? (o->until > o->skip ? (long long)(o->until - o->skip < (unsigned long long)room ? o->until - o->skip : (unsigned long long)room) : 0)
                            : room;
        nframes += f->nframes;
        nbytes += f->used;
        cap += (size_t)count[i];
        if (count[i] > most) most = count[i];
    }
    bytes = (uint8_t *)malloc(nbytes ? nbytes : 1);
    sizes = (int *)malloc(sizeof(int) * (size_t)(nframes ? nframes : 1));
    pcm = malloc((cap ? cap : 1) * nch * (narrow ? 2 : 4));
    raw = (uint8_t *)malloc((size_t)(most ? most : 1) * nch * ((like.bits_per_sample + 7) / 8));
    if (!bytes || !sizes || !pcm || !raw) { fprintf(stderr, "out of memory\n"); goto out; }
    {
        size_t at = 0;
        long long fr = 0;
        for (int i = 0; i < n; i++) {
            const flac_in *f = &fs[i];
            if (!fow[i]) continue;
            memcpy(bytes + at, f->file + f->pos, f->used);
            memcpy(sizes + fr, f->sizes, sizeof(int) * (size_t)f->nframes);
            at += f->used;
            fr += f->nframes;
        }
    }
    long long decoded = 0;
    if (flake_amd_decode_set_windows(g, n, fow, bytes, nbytes, sizes, fixed, first, count, pcm, narrow ? 2 : 4, cap, got, status,
                                     &decoded) < 0) {
        fprintf(stderr, "decode error: %s\n", flake_amd_decode_set_last_error(g));
        goto out;
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        flac_in *f = &fs[i];
        if (f->skip) continue;
        f->fo = wav_begin(f->name);
        if (!f->fo) goto out;
        if (got[i] < 0) {
            fprintf(stderr, "%s: the window does not decode (status %d)\n", f->path, status[i]);
            f->bad = 1;
            at += (size_t)count[i];
        } else {
            wav_samples(f->fo, &like, (const char *)pcm + at * nch * (narrow ? 2 : 4), (size_t)got[i], raw);
            f->total = (unsigned long long)got[i];
            at += (size_t)got[i];
        }
        wav_end(f->fo, &like, f->total);
        f->fo = NULL;
        if (!f->bad) fprintf(stderr, "%s: %llu sample-frames decoded\n", f->path, f->total);
    }
    fprintf(stderr, "%lld of %lld frames decoded\n", decoded, nframes);
    rc = any_bad(fs, n);
out:
    if (g) flake_amd_decode_set_close(g);
    free(fow); free(fixed); free(first); free(count); free(got); free(status); free(pieced);
    free(bytes); free(sizes); free(pcm); free(raw);
    flac_free(fs, n);
    return rc;
}

static int run_decode_mode(const opts *o, const char *argv0)
{
    if (!o->setdir && o->npos != 2) {
        if (o->window)
            fprintf(stderr, "usage: %s --decode --skip N --until N in.flac out.wav\n"
                            "       %s --decode --set OUTDIR --skip N --until N a.flac b.flac ...\n", argv0, argv0);
        else
            fprintf(stderr, "usage: %s --decode in.flac out.wav\n       %s --decode --set OUTDIR a.flac b.flac ...\n", argv0, argv0);
        return 2;
    }
    if (o->window) return run_decode_windows(o);
    if (o->setdir) return run_decode_set(o);
    return run_decode(o->pos[0], o->pos[1]);
}

/* ---- the modes, in order of precedence, and the switches each accepts ---- */
enum {
    A_LEVEL = 1,           /* -0..-12 */
    A_BSIZE = 2,           /* -b N */
    A_SET = 4,             /* --set OUTDIR */
    A_SET_FIRST = 8,       /* --set OUTDIR, the first one only */
    A_SYNTH = 16,          /* --synth N, --channels N, --bps N */
    A_STREAMS = 32,        /* --synth-streams N */
    A_VERIFY = 64,         /* --verify */
    A_WINDOW = 128,        /* --skip N, --until N (samples) */
    A_SEEK = 256,          /* --seekpoints N (samples) */
    A_MODE_VALUE = 512     /* the mode's own word takes N: --reseek N */
};

typedef struct {
    const char *word;      /* the mode is on where this word is among the arguments */
    unsigned accepts;
    int (*run)(const opts *o, const char *argv0);
} mode;

static const mode modes[] = {
    {"--reseek", A_SET | A_MODE_VALUE, run_reseek},
    {"--recode", A_LEVEL | A_BSIZE | A_SET | A_VERIFY | A_SEEK, run_recode_set},
    {"--decode", A_SET_FIRST | A_WINDOW, run_decode_mode},
    {"--set", A_LEVEL | A_BSIZE | A_SET | A_SYNTH | A_STREAMS | A_VERIFY | A_SEEK, run_set},
    {NULL, A_LEVEL | A_BSIZE | A_SYNTH | A_VERIFY | A_SEEK, run_encode},
};

int main(int argc, char **argv)
{
    const mode *m = modes;
    int at = argc;                     /* where the mode's word stands first */
    for (; m->word; m++) {
        for (at = 1; at < argc && strcmp(argv[at], m->word); at++) ;
        if (at < argc) break;
    }
    opts o;
    memset(&o, 0, sizeof o);
    o.level = 5; o.bsize = -1; o.channels = 2; o.bps = 16;
    o.pos = (char **)calloc((size_t)argc, sizeof(char *));
    if (!o.pos) return 1;
    unsigned acc = m->accepts;
    int seek_bad = 0;                  /* --seekpoints where it cannot be, or without a count of at least 1 */
    /* a switch that the mode does not accept, or one whose value is missing, is a positional argument; so is every
     * other word but the mode's own */
    for (int i = 1; i < argc; i++) {
        const char *w = argv[i];
        const int val = i + 1 < argc;
        if ((acc & A_LEVEL) && w[0] == '-' && w[1] >= '0' && w[1] <= '9') o.level = atoi(w + 1);
        else if ((acc & A_BSIZE) && val && !strcmp(w, "-b")) o.bsize = atoi(argv[++i]);
        else if ((acc & (A_SET | A_SET_FIRST)) && val && !strcmp(w, "--set")) { o.setdir = argv[++i]; acc &= ~(unsigned)A_SET_FIRST; }
        else if ((acc & A_SYNTH) && val && !strcmp(w, "--synth")) o.synth = atoi(argv[++i]);
        else if ((acc & A_STREAMS) && val && !strcmp(w, "--synth-streams")) o.synth_streams = atoi(argv[++i]);
        else if ((acc & A_SYNTH) && val && !strcmp(w, "--channels")) o.channels = atoi(argv[++i]);
        else if ((acc & A_SYNTH) && val && !strcmp(w, "--bps")) o.bps = atoi(argv[++i]);
        else if ((acc & A_VERIFY) && !strcmp(w, "--verify")) o.verify = 1;
        else if ((acc & A_WINDOW) && val && !strcmp(w, "--skip")) { o.skip = strtoull(argv[++i], NULL, 10); o.window = 1; }
        else if ((acc & A_WINDOW) && val && !strcmp(w, "--until")) { o.until = strtoull(argv[++i], NULL, 10); o.window = 1; }
        else if (!strcmp(w, "--seekpoints")) {
            o.seekpoints = ((acc & A_SEEK) && val) ? strtoull(argv[++i], NULL, 10) : 0;
            seek_bad |= !o.seekpoints;
        }
        else if (i == at && (acc & A_MODE_VALUE)) o.seekpoints = val ? strtoull(argv[++i], NULL, 10) : 0;
        else if (i != at) {
            o.pos[o.npos++] = argv[i];
            /* (the single-file form: the first word is the input unless --synth came before it, the last the output) */
            if (!o.in && !o.synth) o.in = w; else o.out = w;
        }
    }
    if (seek_bad) fprintf(stderr, SEEK_USAGE, argv[0], argv[0]);
    const int rc = seek_bad ? 2 : m->run(&o, argv[0]);
    free(o.pos);
    return rc;
}
