/*
 * s5skim.c — `slow5tools skim` (src/skim.c) on the GPU press path: every field of every read but the raw signal.
 *
 *   s5skim [--rid | --hdr] [-K batch] in.blow5
 *       (default)  a column line, then one line per record in file order (src/skim.c:340-420).  The file is read in chunks straight
 *                  into pinned memory and framed in place; at most K records (default 4096, src/cmd.h) go to one s5gpu_skim_stream call,
 *                  which inflates them on the device, formats the lines there and returns them as one block of text.
 *       --rid      the read ids, one per line, in file order (src/skim.c:31-51).  Ids come from the device id path
 *                  (s5gpu_record_ids_stream; zstd records and ids longer than its pitch take the default mode's path); no .idx file is
 *                  written.  A repeated id is an error, as slow5_idx_load makes it in the reference.
 *       --hdr      the header as SLOW5 ASCII (src/skim.c:54-57).
 *   Output goes to stdout.  SLOW5 ASCII input is refused.  S5SKIM_CHUNK_KB (tests): the chunk size.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

static int die(const char *what) {
    fprintf(stderr, "s5skim: %s (%s)\n", what, s5gpu_last_error());
    return EXIT_FAILURE;
}
static int rec_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_ZLIB ? S5GPU_REC_ZLIB : m == SLOW5_COMPRESS_ZSTD ? S5GPU_REC_ZSTD : S5GPU_REC_NONE; }
static int sig_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_SVB_ZD ? S5GPU_SIG_SVB_ZD : m == SLOW5_COMPRESS_EX_ZD ? S5GPU_SIG_EX_ZD : S5GPU_SIG_NONE; }

/* the records of the file, a chunk at a time: [u64 size][bytes] framed in place, a record the chunk's end cuts carried to the next */
typedef struct {
    FILE *fp;
    uint64_t pos, end;           /* file offset of the next unread byte; of the end-of-file marker */
    uint8_t *buf;                /* pinned */
    size_t cap, have, used;      /* bytes in buf; bytes of buf already handed out */
    uint64_t *rec_pos;
    uint32_t *rec_len;
    uint32_t K;
} reader_t;

static int refill(reader_t *R, size_t need) {
    const size_t keep = R->have - R->used;
    if (need > R->cap) {                                   /* a record larger than the chunk: a larger buffer */
        size_t cap = R->cap;
        while (cap < need) cap *= 2;
        uint8_t *b = (uint8_t *)s5gpu_host_alloc(cap + 64);
        if (!b) return -1;
        memcpy(b, R->buf + R->used, keep);
        s5gpu_host_free(R->buf);
        R->buf = b;
        R->cap = cap;
    } else if (keep) {
        memmove(R->buf, R->buf + R->used, keep);
    }
    R->have = keep;
    R->used = 0;
    uint64_t want = R->cap - R->have;
    if (want > R->end - R->pos) want = R->end - R->pos;
    if (want && fread(R->buf + R->have, 1, (size_t)want, R->fp) != want) return -1;
    R->pos += want;
    R->have += (size_t)want;
    return 0;
}

/* frames up to K records of the buffer: their count, 0 at the end of the records, -1 on a damaged file */
static int64_t next_batch(reader_t *R) {
    uint32_t n = 0;
    size_t p = R->used;
    for (;;) {
        while (n < R->K && p + 8 <= R->have) {
            uint64_t sz;
            memcpy(&sz, R->buf + p, 8);
            if (sz > 0xFFFFFF00ull) return -1;
            if (p + 8 + sz > R->have) break;
            R->rec_pos[n] = p + 8;
            R->rec_len[n] = (uint32_t)sz;
            n++;
            p += 8 + sz;
        }
        if (n || R->pos == R->end) break;
        /* nothing framed: the next record is cut by the chunk's end (or the buffer is empty) */
        size_t need = R->have - R->used;
        if (need >= 8) { uint64_t sz; memcpy(&sz, R->buf + R->used, 8); need = 8 + sz; }
        if (refill(R, need < R->cap ? R->cap : need) != 0) return -1;
        p = R->used;
    }
    if (n == 0 && R->have != R->used) return -1;           /* bytes left over that make no record */
    R->used = p;
    return n;
}

/* the records of the batch that follows: rec_pos[] point into R->buf, valid until the next next_batch */
static int reader_open(reader_t *R, slow5_file_t *in, const char *path, uint32_t K, size_t chunk) {
    memset(R, 0, sizeof *R);
    struct stat st;
    if (stat(path, &st) != 0 || (uint64_t)st.st_size < in->meta.start_rec_offset + 5) return -1;
    char eof[5];
    R->fp = in->fp;
    if (fseeko(R->fp, (off_t)st.st_size - 5, SEEK_SET) != 0 || fread(eof, 1, 5, R->fp) != 5 || memcmp(eof, "5WOLB", 5) != 0) return -1;
    if (fseeko(R->fp, (off_t)in->meta.start_rec_offset, SEEK_SET) != 0) return -1;
    R->pos = in->meta.start_rec_offset;
    R->end = (uint64_t)st.st_size - 5;
    R->cap = chunk;
    R->buf = (uint8_t *)s5gpu_host_alloc(chunk + 64);
    R->K = K;
    R->rec_pos = (uint64_t *)malloc(sizeof(uint64_t) * K);
    R->rec_len = (uint32_t *)malloc(sizeof(uint32_t) * K);
    return R->buf && R->rec_pos && R->rec_len ? 0 : -1;
}

typedef struct {                 /* growable host buffer for the lines of one call */
    uint8_t *p;
    size_t cap;
    uint64_t *off;
    int32_t *status;
} lines_t;

/* the lines of a batch (s5gpu_skim_stream, redone once with the room it asked for) */
static int skim_batch(reader_t *R, uint32_t n, int rec, int sig, const s5gpu_skim_layout_t *L, lines_t *o) {
    int rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, rec, sig, L, o->p, o->cap, o->off, o->status);
    if (rc == S5GPU_ERR_NOMEM) {
        const size_t need = (size_t)o->off[0];
        s5gpu_host_free(o->p);
        o->cap = need + need / 4;
        o->p = (uint8_t *)s5gpu_host_alloc(o->cap);
        if (!o->p) return S5GPU_ERR_NOMEM;
        rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, rec, sig, L, o->p, o->cap, o->off, o->status);
    }
    if (rc == S5GPU_ERR_DATA) {
        for (uint32_t i = 0; i < n; i++)
            if (o->status[i]) { fprintf(stderr, "s5skim: record %u of the batch cannot be skimmed (status %d)\n", i, o->status[i]); break; }
    }
    return rc;
}

/* ---- --rid: ids in file order, a repeated one is an error ---- */
typedef struct { char *ids; size_t len, cap; uint64_t *at; uint64_t n, ncap; } idlist_t;
static int id_add(idlist_t *I, const char *id, size_t l) {
    if (I->len + l + 1 > I->cap) { I->cap = (I->cap + l + 1) * 2; I->ids = (char *)realloc(I->ids, I->cap); if (!I->ids) return -1; }
    if (I->n + 2 > I->ncap) { I->ncap = (I->ncap + 2) * 2; I->at = (uint64_t *)realloc(I->at, sizeof(uint64_t) * I->ncap); if (!I->at) return -1; }
    I->at[I->n++] = I->len;
    memcpy(I->ids + I->len, id, l);
    I->len += l;
    I->ids[I->len++] = '\n';
    I->at[I->n] = I->len;
    return 0;
}
static uint64_t hash_id(const char *p, size_t l) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < l; i++) h = (h ^ (uint8_t)p[i]) * 1099511628211ull;
    return h;
}
/* the first id that occurs twice, or -1 */
static int64_t first_duplicate(const idlist_t *I) {
    uint64_t cap = 16;
    while (cap < 2 * I->n) cap *= 2;
    int64_t *tab = (int64_t *)malloc(sizeof(int64_t) * cap);
    if (!tab) return -2;
    for (uint64_t s = 0; s < cap; s++) tab[s] = -1;
    int64_t dup = -1;
    for (uint64_t i = 0; i < I->n && dup < 0; i++) {
        const char *p = I->ids + I->at[i];
        const size_t l = I->at[i + 1] - I->at[i] - 1;
        for (uint64_t s = hash_id(p, l) & (cap - 1);; s = (s + 1) & (cap - 1)) {
            if (tab[s] < 0) { tab[s] = (int64_t)i; break; }
            const uint64_t j = (uint64_t)tab[s];
            if (I->at[j + 1] - I->at[j] - 1 == l && memcmp(I->ids + I->at[j], p, l) == 0) { dup = (int64_t)i; break; }
        }
    }
    free(tab);
    return dup;
}

/* --rid's layout: the aux fields' types only, every role "." — a line is only needed for its first column, and the reference's --rid
 * reads the index alone, so a known field declared with another type is no error here (the default mode refuses it) */
static int rid_layout(const char *h, size_t len, s5gpu_skim_layout_t *L) {
    size_t b = 0;
    while (b < len) {
        const char *e = (const char *)memchr(h + b, '\n', len - b);
        const size_t l = e ? (size_t)(e - h) - b : len - b;
        if (l >= 6 && memcmp(h + b, "#char*", 6) == 0) {
            const int k = s5gpu_aux_types_parse(h + b, l, L->type, S5GPU_SKIM_MAX_AUX);
            if (k < 0) return -1;
            L->n_aux = (uint32_t)k;
            for (int a = 0; a < k; a++) L->role[a] = S5GPU_SKIM_DOT;
            L->n_unhandled = (uint32_t)k;
            return 0;
        }
        b += l + 1;
    }
    return -1;
}

int main(int argc, char **argv) {
    int rid = 0, hdr = 0;
    long K = 4096;
    const char *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--rid")) rid = 1;
        else if (!strcmp(argv[i], "--hdr")) hdr = 1;
        else if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else { path = NULL; break; }
    }
    if (!path || K < 1 || K > (1l << 24)) {
        fprintf(stderr, "usage: s5skim [--rid | --hdr] [-K batch] in.blow5\n");
        return EXIT_FAILURE;
    }
    if (rid && hdr) { fprintf(stderr, "s5skim: --rid and --hdr cannot be used together\n"); return EXIT_FAILURE; }
    slow5_file_t *in = slow5_open(path, "r");
    if (!in) { fprintf(stderr, "s5skim: cannot open %s\n", path); return EXIT_FAILURE; }
    if (in->format != SLOW5_FORMAT_BINARY) { fprintf(stderr, "s5skim: %s is SLOW5 ASCII; s5skim reads BLOW5 files only\n", path); return EXIT_FAILURE; }
    if (hdr) {
        const slow5_press_method_t none = {SLOW5_COMPRESS_NONE, SLOW5_COMPRESS_NONE};
        if (slow5_hdr_fwrite(stdout, in->header, SLOW5_FORMAT_ASCII, none) < 0 || fflush(stdout) != 0) return die("cannot write the header");
        slow5_close(in);
        return EXIT_SUCCESS;
    }
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    s5gpu_skim_layout_t *L = (s5gpu_skim_layout_t *)calloc(1, sizeof *L);
    if (!L) return die("out of memory");
    if (rid ? rid_layout(in->header->data, in->header->data_len, L) != 0
            : s5gpu_skim_layout_parse(in->header->data, in->header->data_len, L) != S5GPU_OK)
        return die("the header cannot be skimmed");
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    size_t chunk = (size_t)64 << 20;
    const char *e = getenv("S5SKIM_CHUNK_KB");
    if (e && atoi(e) > 0) chunk = (size_t)atoi(e) << 10;
    reader_t R;
    if (reader_open(&R, in, path, (uint32_t)K, chunk) != 0) return die("cannot read the records (no end-of-file marker, or out of memory)");
    lines_t o;
    o.cap = (size_t)K * 256 + 4096;
    o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
    o.off = (uint64_t *)malloc(sizeof(uint64_t) * (K + 1));
    o.status = (int32_t *)malloc(sizeof(int32_t) * K);
    if (!o.p || !o.off || !o.status) return die("out of memory");

    if (rid) {
        enum { PITCH = 128 };
        char *ids = (char *)malloc((size_t)K * PITCH);
        uint16_t *id_len = (uint16_t *)malloc(sizeof(uint16_t) * K);
        int32_t *st = (int32_t *)malloc(sizeof(int32_t) * K);
        idlist_t I;
        memset(&I, 0, sizeof I);
        if (!ids || !id_len || !st) return die("out of memory");
        for (;;) {
            const int64_t n = next_batch(&R);
            if (n < 0) return die("damaged record framing");
            if (n == 0) break;
            int need_lines = rec == S5GPU_REC_ZSTD;
            if (!need_lines) {
                if (s5gpu_record_ids_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, PITCH, ids, id_len, st) != S5GPU_OK) return die("read ids failed");
                for (int64_t i = 0; i < n; i++) if (st[i]) need_lines = 1;
            }
            if (need_lines) {                              /* zstd records, long ids: the id is the first column of the skim line */
                if (skim_batch(&R, (uint32_t)n, rec, sig, L, &o) != S5GPU_OK) return die("skim failed");
            }
            for (int64_t i = 0; i < n; i++) {
                int rc;
                if (rec != S5GPU_REC_ZSTD && st[i] == 0) rc = id_add(&I, ids + (size_t)i * PITCH, id_len[i]);
                else {
                    const char *line = (const char *)o.p + o.off[i];
                    const char *tab = (const char *)memchr(line, '\t', o.off[i + 1] - o.off[i]);
                    rc = tab ? id_add(&I, line, (size_t)(tab - line)) : -1;
                }
                if (rc) return die("out of memory");
            }
        }
        const int64_t dup = first_duplicate(&I);
        if (dup == -2) return die("out of memory");
        if (dup >= 0) {
            fprintf(stderr, "s5skim: read id '%.*s' occurs more than once in %s\n", (int)(I.at[dup + 1] - I.at[dup] - 1), I.ids + I.at[dup], path);
            return EXIT_FAILURE;
        }
        if (I.len && fwrite(I.ids, 1, I.len, stdout) != I.len) return die("write failed");
        if (fflush(stdout) != 0) return die("write failed");
        return EXIT_SUCCESS;
    }

    /* default: the column line, a warning per field skim does not handle (src/skim.c:257), then the records */
    for (uint32_t a = 0; a < L->n_aux; a++)
        if (L->role[a] == S5GPU_SKIM_DOT)
            fprintf(stderr, "[WARNING] s5skim: Field '%.*s' is not yet handled or not present in the input file. A '.' will be printed\n",
                    (int)L->name_len[a], L->text + L->name_off[a]);
    fputs("#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal", stdout);
    for (uint32_t a = 0; a < L->n_aux; a++) printf("\t%.*s", (int)L->name_len[a], L->text + L->name_off[a]);
    fputc('\n', stdout);
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) return die("damaged record framing");
        if (n == 0) break;
        if (skim_batch(&R, (uint32_t)n, rec, sig, L, &o) != S5GPU_OK) return die("skim failed");
        if (o.off[n] && fwrite(o.p, 1, o.off[n], stdout) != o.off[n]) return die("write failed");
    }
    if (fflush(stdout) != 0) return die("write failed");
    return EXIT_SUCCESS;
}
