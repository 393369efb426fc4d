/*
 * s5tool.h — what the tools of this directory share, so that each keeps only what is its own: its usage text, its options, its one library
 * call and its output lines.  Plain C11, `static inline` functions only: a tool stays one gcc line and uses the part it needs.
 *
 *   #define _GNU_SOURCE            (getline, fseeko: as every tool does, before its first include)
 *   #define S5TOOL "s5events"      the tool's name: the prefix of every message
 *   #define S5TOOL_DIE 2           (optional) die(what) = complain(what), then this value: the tool's code for an error
 *   #include "s5tool.h"
 *
 *   1. small pieces     complain / die, rec_code_of / sig_code_of, rid_layout, read_reference, event_params, open_blow5, big_stdout
 *   2. batch_t          up to K records of slow5_get_next_mem at a time, and their read ids (s5events, s5map, s5align, s5pileup, s5refine,
 *                       s5extend; s5contrast without the ids)
 *   3. reader_t         the records of a BLOW5 file a chunk at a time, framed in place (s5skim, s5sum, s5diff, s5stats), idsrc_t their ids,
 *                       and textbatch_t the record lines of a SLOW5 ASCII file (s5sum, s5stats)
 *   4. xxh64            the header digest (s5sum, s5diff)
 *   5. idlist_t         a growable list of read ids and an open-addressed table over it (s5skim, s5sum, s5diff)
 *
 * A function that fails has said why on stderr and returns -1 (or NULL) unless its comment says otherwise.
 */
#ifndef S5TOOL_H
#define S5TOOL_H

#ifndef S5TOOL
#error "define S5TOOL, the tool's name in its messages, before s5tool.h is included"
#endif

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

/* ---- 1. small pieces ---- */

static inline void complain(const char *what) { fprintf(stderr, S5TOOL ": %s (%s)\n", what, s5gpu_last_error()); }
#ifdef S5TOOL_DIE
static inline int die(const char *what) {
    complain(what);
    return S5TOOL_DIE;
}
#endif

static inline int rec_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_ZLIB ? S5GPU_REC_ZLIB : m == SLOW5_COMPRESS_ZSTD ? S5GPU_REC_ZSTD : S5GPU_REC_NONE; }
static inline int sig_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_SVB_ZD ? S5GPU_SIG_SVB_ZD : m == SLOW5_COMPRESS_EX_ZD ? S5GPU_SIG_EX_ZD : S5GPU_SIG_NONE; }

/* the layout of `s5skim --rid`: the aux fields' types only, every role "." — a skim line that is only needed for its first column.  The
 * reference's --rid reads the index alone, so a known field declared with another type is no error here (s5skim's default mode refuses it).
 * -1, silently: the header text h has no `#char*` line, or one that does not parse */
static inline int rid_layout(const char *h, size_t len, s5gpu_skim_layout_t *L) {
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

/* a reference squiggle: one number per line in strtod syntax, empty lines and lines that start with '#' skipped.  NULL when the file cannot
 * be read, a line is no number, or it holds no number or more than `most` (too_many: how the message words that) */
static inline float *read_reference(const char *path, size_t most, const char *too_many, size_t *n_out) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, S5TOOL ": cannot open %s\n", path); return NULL; }
    size_t n = 0, cap = 1024, line_cap = 0, line_no = 0;
    float *v = (float *)malloc(sizeof(float) * cap);
    char *line = NULL;
    ssize_t l;
    while (v && (l = getline(&line, &line_cap, f)) >= 0) {
        line_no++;
        while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r' || line[l - 1] == ' ' || line[l - 1] == '\t')) line[--l] = 0;
        if (l == 0 || line[0] == '#') continue;
        char *end = NULL;
        const double x = strtod(line, &end);
        if (end == line || *end != 0) {
            fprintf(stderr, S5TOOL ": %s line %zu is not a number\n", path, line_no);
            free(v); free(line); fclose(f);
            return NULL;
        }
        if (n == cap) {
            cap *= 2;
            float *w = (float *)realloc(v, sizeof(float) * cap);
            if (!w) free(v);
            v = w;
        }
        if (v) v[n++] = (float)x;
    }
    free(line);
    fclose(f);
    if (!v) { fprintf(stderr, S5TOOL ": out of memory\n"); return NULL; }
    if (n == 0 || n > most) { fprintf(stderr, S5TOOL ": %s holds %s\n", path, n ? too_many : "no number"); free(v); return NULL; }
    *n_out = n;
    return v;
}

/* the event detector's parameters: DNA 3, 6, 1.4, 9.0, 0.2; RNA 7, 14, 2.5, 9.0, 1.0 */
static inline const s5gpu_event_params_t *event_params(int rna) {
    static const s5gpu_event_params_t dna = {3, 6, 1.4, 9.0, 0.2}, rnap = {7, 14, 2.5, 9.0, 1.0};
    return rna ? &rnap : &dna;
}

/* a BLOW5 file, open; SLOW5 text (told from BLOW5 by the file's first bytes) is refused: "<path> <text_is>", NULL for the common wording */
static inline slow5_file_t *open_blow5(const char *path, const char *text_is) {
    slow5_file_t *in = slow5_open(path, "r");
    if (!in) { fprintf(stderr, S5TOOL ": cannot open %s\n", path); return NULL; }
    if (in->format != SLOW5_FORMAT_BINARY) {
        fprintf(stderr, S5TOOL ": %s %s\n", path, text_is ? text_is : "is SLOW5 text: convert it to BLOW5 first");
        slow5_close(in);
        return NULL;
    }
    return in;
}

/* stdout through a 1 MiB buffer: the tools print a line per event */
static inline void big_stdout(void) {
    static char obuf[1 << 20];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
}

enum { S5_ID_PITCH = 128 };              /* the device id path's room per read id; a longer id comes from a skim line */

/* the read ids of n records framed in buf ([u64 size][bytes], record i at rec_pos[i]): ist[i] = 0 and the id at ids + i * S5_ID_PITCH, or
 * ist[i] != 0 where the device id path leaves the id to a skim line (an id longer than the pitch, a record it cannot read) */
static inline int framed_ids(uint32_t n, const uint8_t *buf, size_t have, const uint64_t *rec_pos, const uint32_t *rec_len, int rec, char *ids,
                             uint16_t *id_len, int32_t *ist) {
    if (s5gpu_record_ids_stream(n, buf, have, rec_pos, rec_len, rec, S5_ID_PITCH, ids, id_len, ist) == S5GPU_OK) return 0;
    complain("read ids failed");
    return -1;
}

/* ---- 2. the record batch: up to K records at a time from slow5_get_next_mem, for the calls that take records anywhere in host memory ----
 *
 *   batch_open(&B, in, path, K);
 *   while ((n = batch_next(&B)) > 0) {
 *       the library call over B.mem, B.len -> st[]
 *       batch_ids(&B, st, corrupt, 0);  then per record i: batch_id(&B, i, &idl), batch_corrupt(&B, i, st[i]) or the tool's own lines
 *       batch_release(&B);
 *   }
 *   n < 0: an error;  batch_close(&B);
 */
typedef struct {
    slow5_file_t *in;
    const char *path;
    uint32_t K, n;               /* records of a batch at most; of this one */
    int rec, sig;                /* the file's presses as S5GPU_REC_* / S5GPU_SIG_* */
    int at_end, path_in_messages;/* (s5contrast reads two files: its "too large" line names the file) */
    uint64_t n_done;             /* records of the batches released so far */
    size_t bytes;                /* of this batch, with the 8 bytes of framing each */
    void **mem;                  /* record i: mem[i], len[i] bytes, malloc'd */
    size_t *len;
    /* the ids */
    uint8_t *chunk;              /* pinned: the records framed in one buffer for the device id path */
    size_t chunk_cap;
    uint64_t *rec_pos;
    uint32_t *rec_len;
    int32_t *ist;
    char *ids;
    uint16_t *id_len;
    s5gpu_skim_layout_t *L;      /* rid_layout, made when the first skim line is needed */
    void **line;                 /* the skim line of record i, or NULL */
    size_t *line_len;
} batch_t;

static inline int batch_open(batch_t *B, slow5_file_t *in, const char *path, long K) {
    memset(B, 0, sizeof *B);
    B->in = in;
    B->path = path;
    B->K = (uint32_t)K;
    B->rec = rec_code_of(in->compress->record_press->method);
    B->sig = sig_code_of(in->compress->signal_press->method);
    B->mem = (void **)calloc((size_t)K, sizeof(void *));
    B->len = (size_t *)malloc(sizeof(size_t) * (size_t)K);
    B->rec_pos = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)K);
    B->rec_len = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)K);
    B->ist = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    B->ids = (char *)malloc((size_t)K * S5_ID_PITCH);
    B->id_len = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)K);
    B->line = (void **)calloc((size_t)K, sizeof(void *));
    B->line_len = (size_t *)malloc(sizeof(size_t) * (size_t)K);
    if (B->mem && B->len && B->rec_pos && B->rec_len && B->ist && B->ids && B->id_len && B->line && B->line_len) return 0;
    complain("out of memory");
    return -1;
}

/* the next batch: its record count, 0 behind the last record, -1 on a record that cannot be read or is too large */
static inline int64_t batch_next(batch_t *B) {
    B->n = 0;
    B->bytes = 0;
    while (!B->at_end && B->n < B->K) {
        const uint32_t n = B->n;
        B->mem[n] = slow5_get_next_mem(&B->len[n], B->in);
        if (!B->mem[n]) {
            if (slow5_errno != SLOW5_ERR_EOF) { fprintf(stderr, S5TOOL ": cannot read record %" PRIu64 " of %s\n", B->n_done + n, B->path); return -1; }
            B->at_end = 1;
            break;
        }
        if (B->len[n] > 0xFFFFFF00u) {
            if (B->path_in_messages) fprintf(stderr, S5TOOL ": record %" PRIu64 " of %s is too large\n", B->n_done + n, B->path);
            else fprintf(stderr, S5TOOL ": record %" PRIu64 " is too large\n", B->n_done + n);
            return -1;
        }
        B->bytes += 8 + B->len[n];
        B->n++;
    }
    return B->n;
}

/* the read ids of the batch: the device id path over the records framed in one buffer; what it leaves (zstd records, long ids) is the first
 * column of a skim line.  st: the library call's status per record; corrupt(st[i]): the decoder refused record i, which has no skim line
 * either.  only_named: the tool names a read only where st[i] != 0 (s5pileup): a batch without one makes no id call at all */
static inline int batch_ids(batch_t *B, const int32_t *st, int (*corrupt)(int32_t), int only_named) {
    const uint32_t n = B->n;
    int named = !only_named;
    for (uint32_t i = 0; i < n; i++) {
        named |= st[i] != 0;
        B->ist[i] = 5;
        B->line[i] = NULL;
    }
    if (named && B->rec != S5GPU_REC_ZSTD) {
        if (B->bytes + 64 > B->chunk_cap) {
            if (B->chunk) s5gpu_host_free(B->chunk);
            B->chunk_cap = B->bytes + B->bytes / 4 + 64;
            B->chunk = (uint8_t *)s5gpu_host_alloc(B->chunk_cap);
            if (!B->chunk) { B->chunk_cap = 0; complain("out of memory"); return -1; }
        }
        size_t p = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t sz = B->len[i];
            memcpy(B->chunk + p, &sz, 8);
            memcpy(B->chunk + p + 8, B->mem[i], B->len[i]);
            B->rec_pos[i] = p + 8;
            B->rec_len[i] = (uint32_t)B->len[i];
            p += 8 + B->len[i];
        }
        if (framed_ids(n, B->chunk, p, B->rec_pos, B->rec_len, B->rec, B->ids, B->id_len, B->ist) != 0) return -1;
    }
    for (uint32_t i = 0; i < n; i++) {
        if ((only_named && st[i] == 0) || B->ist[i] == 0 || corrupt(st[i])) continue;
        if (!B->L) {
            B->L = (s5gpu_skim_layout_t *)calloc(1, sizeof *B->L);
            if (!B->L) { complain("out of memory"); return -1; }
            if (rid_layout(B->in->header->data, B->in->header->data_len, B->L) != 0) { complain("the header names no column types"); return -1; }
        }
        const void *r1 = B->mem[i];
        int32_t s1 = 0;
        if (s5gpu_skim_batch(1, &r1, &B->len[i], B->rec, B->sig, B->L, &B->line[i], &B->line_len[i], &s1) != S5GPU_OK || !B->line[i]) {
            complain("read ids failed");
            return -1;
        }
    }
    return 0;
}

/* the id of record i behind batch_ids, *idl bytes; NULL: it has none (a corrupt record the id path could not read, a read not named) */
static inline const char *batch_id(const batch_t *B, uint32_t i, size_t *idl) {
    *idl = 0;
    if (B->ist[i] == 0) { *idl = B->id_len[i]; return B->ids + (size_t)i * S5_ID_PITCH; }
    if (!B->line[i]) return NULL;
    const char *id = (const char *)B->line[i], *tab = (const char *)memchr(id, '\t', B->line_len[i]);
    *idl = tab ? (size_t)(tab - id) : B->line_len[i];
    return id;
}

/* a corrupt record goes to stderr by its read id, or by its number in the file when the id cannot be read */
static inline void batch_corrupt(const batch_t *B, uint32_t i, int32_t status) {
    size_t idl;
    const char *id = batch_id(B, i, &idl);
    if (id) fprintf(stderr, S5TOOL ": read %.*s is corrupt (status %d)\n", (int)idl, id, status);
    else fprintf(stderr, S5TOOL ": record %" PRIu64 " of the file is corrupt (status %d)\n", B->n_done + i, status);
}

static inline void batch_release(batch_t *B) {
    for (uint32_t i = 0; i < B->n; i++) {
        free(B->line[i]);
        free(B->mem[i]);
        B->line[i] = B->mem[i] = NULL;
    }
    B->n_done += B->n;
    B->n = 0;
}

/* (the file stays open: it is the caller's) */
static inline void batch_close(batch_t *B) {
    batch_release(B);
    if (B->chunk) s5gpu_host_free(B->chunk);
    free(B->mem); free(B->len); free(B->rec_pos); free(B->rec_len); free(B->ist); free(B->ids); free(B->id_len); free(B->line); free(B->line_len);
    free(B->L);
}

/* ---- 3. the records of a BLOW5 file, a chunk at a time: [u64 size][bytes] framed in place, a record the chunk's end cuts carried over.
 * pinned: the chunk buffer comes from s5gpu_host_alloc (it goes to the device); else from malloc, and no GPU call is made.  These are
 * silent: -1 is a file without the end-of-file marker, damaged framing, or no memory, and the tool words it ---- */
typedef struct {
    FILE *fp;
    uint64_t pos, end;           /* file offset of the next unread byte; of the end-of-file marker */
    uint8_t *buf;
    size_t cap, have, used;      /* bytes in buf; bytes of buf already handed out */
    uint64_t *rec_pos;           /* of the batch that next_batch framed: offsets into buf, valid until the next next_batch */
    uint32_t *rec_len;
    uint32_t K;
    int pinned;
} reader_t;

static inline uint8_t *chunk_alloc(int pinned, size_t bytes) { return (uint8_t *)(pinned ? s5gpu_host_alloc(bytes) : malloc(bytes)); }
static inline void chunk_free(int pinned, uint8_t *p) { if (pinned) s5gpu_host_free(p); else free(p); }

static inline int refill(reader_t *R, size_t need) {
    const size_t keep = R->have - R->used;
    if (need > R->cap) {                                   /* a record larger than the chunk: a larger buffer */
        size_t cap = R->cap;
        while (cap < need) cap *= 2;
        uint8_t *b = chunk_alloc(R->pinned, cap + 64);
        if (!b) return -1;
        memcpy(b, R->buf + R->used, keep);
        chunk_free(R->pinned, R->buf);
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
static inline int64_t next_batch(reader_t *R) {
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
        if (need >= 8) { uint64_t sz; memcpy(&sz, R->buf + R->used, 8); if (sz > 0xFFFFFF00ull) return -1; need = 8 + sz; }
        if (need > R->have - R->used + (R->end - R->pos)) return -1;   /* the record runs past the end-of-file marker: refused before any buffer grows */
        if (refill(R, need < R->cap ? R->cap : need) != 0) return -1;
        p = R->used;
    }
    if (n == 0 && R->have != R->used) return -1;           /* bytes left over that make no record */
    R->used = p;
    return n;
}
/* the file offset of the byte at buffer offset p */
static inline uint64_t file_offset(const reader_t *R, uint64_t p) { return R->pos - R->have + p; }

static inline int reader_open(reader_t *R, slow5_file_t *in, const char *path, uint32_t K, size_t chunk, int pinned) {
    memset(R, 0, sizeof *R);
    R->pinned = pinned;
    struct stat st;
    if (stat(path, &st) != 0 || (uint64_t)st.st_size < in->meta.start_rec_offset + 5) return -1;
    char eof[5];
    R->fp = in->fp;
    if (fseeko(R->fp, (off_t)st.st_size - 5, SEEK_SET) != 0 || fread(eof, 1, 5, R->fp) != 5 || memcmp(eof, "5WOLB", 5) != 0) return -1;
    if (fseeko(R->fp, (off_t)in->meta.start_rec_offset, SEEK_SET) != 0) return -1;
    R->pos = in->meta.start_rec_offset;
    R->end = (uint64_t)st.st_size - 5;
    if (chunk > R->end - R->pos + 4096) chunk = (size_t)(R->end - R->pos) + 4096;   /* a small file does not need the whole chunk */
    R->cap = chunk;
    R->buf = chunk_alloc(R->pinned, chunk + 64);
    R->K = K;
    R->rec_pos = (uint64_t *)malloc(sizeof(uint64_t) * K);
    R->rec_len = (uint32_t *)malloc(sizeof(uint32_t) * K);
    return R->buf && R->rec_pos && R->rec_len ? 0 : -1;
}
static inline void reader_close(reader_t *R) {
    if (R->buf) chunk_free(R->pinned, R->buf);
    free(R->rec_pos);
    free(R->rec_len);
}

/* the skim lines of the batch the reader framed, as one block of text: line i at p + off[i], off[i + 1] - off[i] bytes with its newline.
 * status may be NULL */
typedef struct {
    uint8_t *p;                  /* pinned, growable */
    size_t cap;
    uint64_t *off;
    int32_t *status;
} lines_t;

/* s5gpu_skim_stream, redone once with the room it asked for; silent: the call's S5GPU_* code */
static inline int skim_lines(const reader_t *R, uint32_t n, int rec, int sig, const s5gpu_skim_layout_t *L, lines_t *o) {
    int rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, rec, sig, L, o->p, o->cap, o->off, o->status);
    if (rc == S5GPU_ERR_NOMEM) {
        const size_t need = (size_t)o->off[0];
        s5gpu_host_free(o->p);
        o->cap = need + need / 4;
        o->p = (uint8_t *)s5gpu_host_alloc(o->cap);
        if (!o->p) return S5GPU_ERR_NOMEM;
        rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, rec, sig, L, o->p, o->cap, o->off, o->status);
    }
    return rc;
}

/* the read ids of the reader's batches: the device id path; zstd records and ids longer than its pitch are the first column of a skim line */
typedef struct {
    slow5_file_t *in;
    int rec, sig;
    uint32_t K;
    char *ids;
    uint16_t *id_len;
    int32_t *st;                 /* 0: the id is in ids; else in the skim line */
    s5gpu_skim_layout_t *L;      /* rid_layout, made with the lines when the first one is needed */
    lines_t txt;
} idsrc_t;

static inline int idsrc_open(idsrc_t *I, slow5_file_t *in, uint32_t K) {
    memset(I, 0, sizeof *I);
    I->in = in;
    I->rec = rec_code_of(in->compress->record_press->method);
    I->sig = sig_code_of(in->compress->signal_press->method);
    I->K = K;
    I->ids = (char *)malloc((size_t)K * S5_ID_PITCH);
    I->id_len = (uint16_t *)malloc(sizeof(uint16_t) * K);
    I->st = (int32_t *)malloc(sizeof(int32_t) * K);
    if (I->ids && I->id_len && I->st) return 0;
    complain("out of memory");
    return -1;
}
static inline void idsrc_close(idsrc_t *I) {
    if (I->txt.p) s5gpu_host_free(I->txt.p);
    free(I->ids); free(I->id_len); free(I->st); free(I->L); free(I->txt.off); free(I->txt.status);
}
/* the ids of the n records the reader has framed; afterwards id_of(I, i, &len).  0; -1; or, silently, the S5GPU_* code of a skim call that
 * failed (S5GPU_ERR_DATA: a corrupt record, I->txt.status says which) */
static inline int idsrc_batch(idsrc_t *I, const reader_t *R, uint32_t n) {
    int need_lines = I->rec == S5GPU_REC_ZSTD;
    if (!need_lines) {
        if (framed_ids(n, R->buf, R->have, R->rec_pos, R->rec_len, I->rec, I->ids, I->id_len, I->st) != 0) return -1;
        for (uint32_t i = 0; i < n; i++) if (I->st[i]) need_lines = 1;
    } else for (uint32_t i = 0; i < n; i++) I->st[i] = 1;
    if (!need_lines) return 0;
    if (!I->txt.p) {
        if (!I->L) {
            I->L = (s5gpu_skim_layout_t *)calloc(1, sizeof *I->L);
            if (!I->L) { complain("out of memory"); return -1; }
            if (rid_layout(I->in->header->data, I->in->header->data_len, I->L) != 0) { complain("the header names no column types"); return -1; }
        }
        I->txt.cap = (size_t)I->K * 256 + 4096;
        I->txt.p = (uint8_t *)s5gpu_host_alloc(I->txt.cap);
        I->txt.off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)I->K + 1));
        I->txt.status = (int32_t *)malloc(sizeof(int32_t) * I->K);
        if (!I->txt.p || !I->txt.off || !I->txt.status) { complain("out of memory"); return -1; }
    }
    const int rc = skim_lines(R, n, I->rec, I->sig, I->L, &I->txt);
    if (rc == S5GPU_ERR_NOMEM && !I->txt.p) { complain("out of memory"); return -1; }
    return rc;
}
static inline const char *id_of(const idsrc_t *I, uint32_t i, size_t *len) {
    if (I->st[i] == 0) { *len = I->id_len[i]; return I->ids + (size_t)i * S5_ID_PITCH; }
    const char *line = (const char *)I->txt.p + I->txt.off[i];
    const char *tab = (const char *)memchr(line, '\t', I->txt.off[i + 1] - I->txt.off[i]);
    *len = tab ? (size_t)(tab - line) : 0;
    return tab ? line : NULL;
}

/* the record lines of a SLOW5 ASCII file, up to K at a time in one buffer (line i at txt + line_pos[i], line_len[i] bytes, 32 zero bytes
 * behind the last), for s5gpu_ascii_to_blow5_stream.  pinned: as the reader's */
typedef struct {
    uint8_t *txt;
    size_t cap, have;
    uint64_t *line_pos;
    uint32_t *line_len;
    uint32_t K;
    char *held;                  /* a line read but not yet placed: the chunk was full */
    size_t held_len;
    int at_end, pinned;
} textbatch_t;

static inline int textbatch_open(textbatch_t *T, uint32_t K, size_t chunk, int pinned) {
    memset(T, 0, sizeof *T);
    T->K = K;
    T->cap = chunk;
    T->pinned = pinned;
    T->txt = chunk_alloc(pinned, chunk + 64);
    T->line_pos = (uint64_t *)malloc(sizeof(uint64_t) * K);
    T->line_len = (uint32_t *)malloc(sizeof(uint32_t) * K);
    if (T->txt && T->line_pos && T->line_len) return 0;
    complain("out of memory");
    return -1;
}
/* the next lines: their count, 0 behind the last, -1 */
static inline int64_t textbatch_next(textbatch_t *T, slow5_file_t *in) {
    uint32_t n = 0;
    T->have = 0;
    while (n < T->K && (!T->at_end || T->held)) {
        if (!T->held) {
            T->held = (char *)slow5_get_next_mem(&T->held_len, in);
            if (!T->held) {
                if (slow5_errno != SLOW5_ERR_EOF) { fprintf(stderr, S5TOOL ": cannot read a record line\n"); return -1; }
                T->at_end = 1;
                break;
            }
        }
        if (T->held_len > 0xFFFFFF00u) { fprintf(stderr, S5TOOL ": a record line is too long\n"); return -1; }
        if (T->have + T->held_len + 32 > T->cap) {
            if (n) break;                                  /* this batch is full: the line opens the next one */
            while (T->have + T->held_len + 32 > T->cap) T->cap *= 2;
            chunk_free(T->pinned, T->txt);
            T->txt = chunk_alloc(T->pinned, T->cap + 64);
            if (!T->txt) { complain("out of memory"); return -1; }
        }
        memcpy(T->txt + T->have, T->held, T->held_len);
        T->line_pos[n] = T->have;
        T->line_len[n] = (uint32_t)T->held_len;
        T->have += T->held_len;
        n++;
        free(T->held);
        T->held = NULL;
    }
    if (n) memset(T->txt + T->have, 0, 32);
    return n;
}
static inline void textbatch_close(textbatch_t *T) {
    if (T->txt) chunk_free(T->pinned, T->txt);
    free(T->held); free(T->line_pos); free(T->line_len);
}

/* ---- 4. XXH64, seed 0 (the published algorithm), for the header text ---- */
static inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static inline uint64_t le64(const uint8_t *p) { uint64_t v = 0; for (int i = 7; i >= 0; i--) v = (v << 8) | p[i]; return v; }
static inline uint64_t le32(const uint8_t *p) { return (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24; }
static inline uint64_t xxh64(const void *data, size_t n) {
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
    const uint8_t *p = (const uint8_t *)data;
    size_t i = 0;
    uint64_t h;
    if (n >= 32) {
        uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
        for (; i + 32 <= n; i += 32)
            for (int k = 0; k < 4; k++) v[k] = rotl64(v[k] + le64(p + i + 8 * k) * P2, 31) * P1;
        h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
        for (int k = 0; k < 4; k++) h = (h ^ (rotl64(v[k] * P2, 31) * P1)) * P1 + P4;
    } else h = P5;
    h += n;
    for (; i + 8 <= n; i += 8) h = rotl64(h ^ (rotl64(le64(p + i) * P2, 31) * P1), 27) * P1 + P4;
    if (i + 4 <= n) { h = rotl64(h ^ (le32(p + i) * P1), 23) * P2 + P3; i += 4; }
    for (; i < n; i++) h = rotl64(h ^ (p[i] * P5), 11) * P1;
    h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
    return h;
}

/* ---- 5. the read ids of a file: NUL-terminated, in file order; a tool keeps what else it knows of read i in arrays of ncap entries of
 * its own, grown when idlist_add has grown ncap ---- */
typedef struct {
    char *ids;
    size_t len, cap;
    uint64_t *at;                /* id i at ids + at[i] */
    uint64_t n, ncap;
} idlist_t;

/* silent: -1 is no memory */
static inline int idlist_add(idlist_t *I, const char *id, size_t l) {
    if (I->len + l + 1 > I->cap) { I->cap = (I->cap + l + 1) * 2; I->ids = (char *)realloc(I->ids, I->cap); if (!I->ids) return -1; }
    if (I->n + 1 > I->ncap) { I->ncap = (I->ncap + 1) * 2; I->at = (uint64_t *)realloc(I->at, sizeof(uint64_t) * I->ncap); if (!I->at) return -1; }
    I->at[I->n++] = I->len;
    memcpy(I->ids + I->len, id, l);
    I->len += l;
    I->ids[I->len++] = '\0';
    return 0;
}
static inline const char *idlist_id(const idlist_t *I, uint64_t i) { return I->ids + I->at[i]; }
static inline uint64_t hash_id(const char *p) {
    uint64_t h = 1469598103934665603ull;
    for (; *p; p++) h = (h ^ (uint8_t)*p) * 1099511628211ull;
    return h;
}
/* an open-addressed table over the ids: the first id that occurs twice, -1: none, -2, silently: out of memory.  The table (slot -> index
 * of the id, -1: free; *tcap slots, a power of two) is the caller's when tab is not NULL */
static inline int64_t idlist_index(const idlist_t *I, int64_t **tab, uint64_t *tcap) {
    uint64_t cap = 16;
    while (cap < 2 * I->n) cap *= 2;
    int64_t *t = (int64_t *)malloc(sizeof(int64_t) * cap);
    if (!t) return -2;
    for (uint64_t s = 0; s < cap; s++) t[s] = -1;
    int64_t dup = -1;
    for (uint64_t i = 0; i < I->n && dup < 0; i++) {
        const char *p = idlist_id(I, i);
        for (uint64_t s = hash_id(p) & (cap - 1);; s = (s + 1) & (cap - 1)) {
            if (t[s] < 0) { t[s] = (int64_t)i; break; }
            if (strcmp(idlist_id(I, (uint64_t)t[s]), p) == 0) { dup = (int64_t)i; break; }
        }
    }
    if (tab) { *tab = t; *tcap = cap; }
    else free(t);
    return dup;
}
/* the index of the NUL-terminated id in the table of idlist_index, or -1 */
static inline int64_t idlist_find(const idlist_t *I, const int64_t *tab, uint64_t tcap, const char *id) {
    for (uint64_t s = hash_id(id) & (tcap - 1);; s = (s + 1) & (tcap - 1)) {
        if (tab[s] < 0) return -1;
        if (strcmp(idlist_id(I, (uint64_t)tab[s]), id) == 0) return tab[s];
    }
}
/* what the tools say of id `dup` of idlist_index */
static inline void complain_duplicate(const idlist_t *I, int64_t dup, const char *path) {
    fprintf(stderr, S5TOOL ": read id '%s' occurs more than once in %s\n", idlist_id(I, (uint64_t)dup), path);
}

#endif
