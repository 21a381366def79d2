/*
 * ref_frames.c -- a libflake CLIENT that writes down everything the library answers.  TEST INFRASTRUCTURE.
 *
 * One source, built twice by oracle/Makefile (target `refframes`), both times on the REFERENCE's own flake.h (and a
 * third time as oracle/ref_frames_own, the subject on this project's own header, for where the reference tree is absent):
 *
 *   _ref/build/ref_frames    linked statically to the reference's own libflake_static.a (its CMake build): THE WITNESS.
 *                            Its frames are the reference's encode.c / optimize.c / vbs.c at work, byte for byte.
 *   _ref/ref_frames_hip      linked to this project's flake_amd/lib/libflake.so: THE SUBJECT, the shipped drop-in
 *                            (host layer -> K0..K4) under the same call sequence.
 *
 * tests/test_ref_witness_cpu.py holds oracle/flake_oracle.c to the witness; tests/test_gpu_ref_witness.py holds the
 * HIP frames to it.  The call sequence is the one flake/flake.c uses: set_defaults, validate_params, encode_init,
 * encode_frame per block, get_streaminfo, write_streaminfo, encode_close.
 *
 *   ref_frames OUT PCM CHANNELS RATE BITS SAMPLES LEVEL [field=value ...] [blocks=n0,n1,...]
 *
 * PCM      raw little-endian int32, interleaved; its length decides how many sample frames there are
 * SAMPLES  FlakeContext.samples (0: unknown)
 * field    any FlakeEncodeParams member but `compression`; members not named keep flake_set_defaults()' value
 * blocks   the block size of every flake_encode_frame() call; without it the PCM goes in params.block_size
 *          blocks and one shorter last call for what remains
 *
 * OUT, all integers little-endian int32:
 *   "FRF1"
 *   validate_params' return value
 *   the 12 FlakeEncodeParams members in flake.h's order, as they stood at flake_encode_init()
 *   flake_encode_init's return value H, then max(H, 0) header bytes
 *   the number of calls C, then per call: block size, return value R, max(R, 0) frame bytes
 *   flake_get_streaminfo's return value, then the 34 bytes flake_write_streaminfo() made of it
 * When validate_params refuses (< 0) the record ends after the parameters; exit status 0 all the same.  Exit status 2:
 * usage; 1: a file could not be read or written.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef REF_FRAMES_OWN_HEADER
/* where the reference tree is absent (oracle/ref_frames_own): libflake's names declared on this project's
 * layout-compatible types, as oracle/dropin_client.c does; only the subject can be built this way */
#include "flake_amd.h"
typedef FlakeAmdContext FlakeContext;
typedef FlakeAmdEncodeParams FlakeEncodeParams;
typedef FlakeAmdStreaminfo FlakeStreaminfo;
int flake_set_defaults(FlakeEncodeParams *params);
int flake_validate_params(const FlakeContext *s);
int flake_encode_init(FlakeContext *s);
void *flake_get_buffer(const FlakeContext *s);
int flake_encode_frame(FlakeContext *s, const int *samples, int block_size);
void flake_encode_close(FlakeContext *s);
int flake_get_streaminfo(const FlakeContext *s, FlakeStreaminfo *si);
void flake_write_streaminfo(const FlakeStreaminfo *si, unsigned char *data);
#else
#include "flake.h"                      /* the reference's header */
#endif

static void put_i32(FILE *f, int v)
{
    unsigned u = (unsigned)v;
    unsigned char b[4] = { (unsigned char)u, (unsigned char)(u >> 8), (unsigned char)(u >> 16), (unsigned char)(u >> 24) };
    fwrite(b, 1, 4, f);
}

static void put_params(FILE *f, const FlakeEncodeParams *p)
{
    put_i32(f, p->compression);
    put_i32(f, p->order_method);
    put_i32(f, p->stereo_method);
    put_i32(f, p->block_size);
    put_i32(f, p->padding_size);
    put_i32(f, p->min_prediction_order);
    put_i32(f, p->max_prediction_order);
    put_i32(f, p->prediction_type);
    put_i32(f, p->min_partition_order);
    put_i32(f, p->max_partition_order);
    put_i32(f, p->variable_block_size);
    put_i32(f, p->allow_vbs);
}

static int *param_field(FlakeEncodeParams *p, const char *name, size_t len)
{
    static const char *const names[] = { "order_method", "stereo_method", "block_size", "padding_size",
        "min_prediction_order", "max_prediction_order", "prediction_type", "min_partition_order",
        "max_partition_order", "variable_block_size", "allow_vbs" };
    int *const fields[] = { &p->order_method, &p->stereo_method, &p->block_size, &p->padding_size,
        &p->min_prediction_order, &p->max_prediction_order, &p->prediction_type, &p->min_partition_order,
        &p->max_partition_order, &p->variable_block_size, &p->allow_vbs };
    for (size_t i = 0; i < sizeof names / sizeof names[0]; i++)
        if (strlen(names[i]) == len && !memcmp(names[i], name, len)) return fields[i];
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc < 8) {
        fprintf(stderr, "usage: ref_frames OUT PCM CHANNELS RATE BITS SAMPLES LEVEL [field=value ...] [blocks=n,n,...]\n");
        return 2;
    }
    FlakeContext s;
    memset(&s, 0, sizeof s);
    s.channels = atoi(argv[3]);
    s.sample_rate = atoi(argv[4]);
    s.bits_per_sample = atoi(argv[5]);
    s.samples = (unsigned)strtoul(argv[6], NULL, 10);
    s.params.compression = atoi(argv[7]);
    if (s.channels < 1 || s.channels > 8) return 2;
    if (flake_set_defaults(&s.params)) {
        fprintf(stderr, "ref_frames: flake_set_defaults refused level %d\n", s.params.compression);
        return 2;
    }
    const char *blocks_arg = NULL;
    for (int a = 8; a < argc; a++) {
        const char *eq = strchr(argv[a], '=');
        if (!eq) { fprintf(stderr, "ref_frames: '%s' is no field=value\n", argv[a]); return 2; }
        if ((size_t)(eq - argv[a]) == 6 && !memcmp(argv[a], "blocks", 6)) { blocks_arg = eq + 1; continue; }
        int *field = param_field(&s.params, argv[a], (size_t)(eq - argv[a]));
        if (!field) { fprintf(stderr, "ref_frames: no parameter '%s'\n", argv[a]); return 2; }
        *field = atoi(eq + 1);
    }

    /* the PCM */
    FILE *fi = fopen(argv[2], "rb");
    if (!fi) { perror(argv[2]); return 1; }
    fseek(fi, 0, SEEK_END);
    const long pcm_bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    const long total = pcm_bytes / (4 * (long)s.channels);        /* sample frames */
    int *pcm = (int *)malloc(pcm_bytes > 0 ? (size_t)pcm_bytes : 1);
    if (!pcm || fread(pcm, 1, (size_t)pcm_bytes, fi) != (size_t)pcm_bytes) { fprintf(stderr, "ref_frames: short read\n"); return 1; }
    fclose(fi);

    FILE *fo = fopen(argv[1], "wb");
    if (!fo) { perror(argv[1]); return 1; }
    fwrite("FRF1", 1, 4, fo);
    const int valid = flake_validate_params(&s);
    put_i32(fo, valid);
    put_params(fo, &s.params);
    if (valid < 0) { fclose(fo); free(pcm); return 0; }

    /* the calls' block sizes */
    const int bs = s.params.block_size;
    long ncalls = 0;
    int *sizes = NULL;
    if (blocks_arg) {
        for (const char *c = blocks_arg; *c; c++) ncalls += (*c == ',');
        ncalls += 1;
        sizes = (int *)malloc(sizeof(int) * (size_t)ncalls);
        const char *c = blocks_arg;
        for (long i = 0; i < ncalls; i++) {
            sizes[i] = atoi(c);
            c = strchr(c, ',');
            if (c) c++;
        }
    } else {
        ncalls = (total + bs - 1) / bs;
        sizes = (int *)malloc(sizeof(int) * (size_t)(ncalls ? ncalls : 1));
        for (long i = 0; i < ncalls; i++) sizes[i] = (int)((i + 1) * bs <= total ? bs : total - i * bs);
    }
    long need = 0;
    for (long i = 0; i < ncalls; i++) {
        if (sizes[i] < 0) { fprintf(stderr, "ref_frames: negative block size\n"); return 2; }
        need += sizes[i];
    }
    if (need > total) { fprintf(stderr, "ref_frames: the blocks ask for %ld sample frames, the file has %ld\n", need, total); return 2; }

    const int hlen = flake_encode_init(&s);
    put_i32(fo, hlen);
    if (hlen > 0) fwrite(s.header, 1, (size_t)hlen, fo);
    put_i32(fo, (int)ncalls);
    if (hlen >= 0) {
        const unsigned char *frame = (const unsigned char *)flake_get_buffer(&s);
        long pos = 0;
        for (long i = 0; i < ncalls; i++) {
            const int fs = flake_encode_frame(&s, pcm + pos * s.channels, sizes[i]);
            put_i32(fo, sizes[i]);
            put_i32(fo, fs);
            if (fs > 0) fwrite(frame, 1, (size_t)fs, fo);
            pos += sizes[i];
        }
    } else {
        for (long i = 0; i < ncalls; i++) { put_i32(fo, sizes[i]); put_i32(fo, -1); }
    }
    FlakeStreaminfo si;
    unsigned char d[34];
    memset(&si, 0, sizeof si);
    memset(d, 0, sizeof d);
    const int sirc = flake_get_streaminfo(&s, &si);
    if (!sirc) flake_write_streaminfo(&si, d);
    put_i32(fo, sirc);
    fwrite(d, 1, 34, fo);
    flake_encode_close(&s);
    const int bad = ferror(fo);
    if (fclose(fo) || bad) { fprintf(stderr, "ref_frames: write failed\n"); return 1; }
    free(sizes);
    free(pcm);
    return 0;
}
