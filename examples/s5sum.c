/*
 * s5sum.c — do two SLOW5 / BLOW5 files hold the same reads?  A content digest per read, hashed on the GPU where the decoder left the read
 * (docs/codecs.md §4.12): the digest does not depend on the record press, the signal press, the file format or the order of the reads.
 *
 *   s5sum [-K batch] file.[b|s]low5
 *       #s5sum\t1\txxh64\t<header digest, 16 hex>
 *       <digest, 16 hex>\t<read_id>              one line per read, file order
 *       #total\t<n>\t<file sum, 16 hex>           the sum of the digests mod 2^64: it does not depend on the order
 *   s5sum [-K batch] --compare a b
 *       header\t<digest a>\t<digest b>            when the header texts differ (does not change the exit code)
 *       only-in-a\t<id> | only-in-b\t<id> | differs\t<id>\t<digest a>\t<digest b>     sorted by id
 *       same\t<number of ids with equal digests>
 *       exit 0 when every id is in both files with equal digests, 1 otherwise
 *   Any error (unreadable or damaged file, corrupt record, an id that occurs twice in one file) exits 2.
 *
 * A BLOW5 file is read in chunks straight into pinned memory and framed in place (the reader of s5skim.c); at most K records (default 4096) go
 * to one s5gpu_digest_stream call: compressed bytes go up, 8 bytes per read come back.  The read ids come from the device id path as in
 * `s5skim --rid`.  A SLOW5 ASCII file (told from BLOW5 by its first bytes) has its lines converted to BLOW5 records with both presses none by
 * s5gpu_ascii_to_blow5_stream, and those go to s5gpu_digest_batch: that path crosses PCIe twice.  The header digest is XXH64 of the header
 * text as BLOW5 stores it (for a .slow5: the ASCII header without its #slow5_version and #num_read_groups lines), made on the host.
 * The digest resists accidents, not adversaries.  S5SUM_CHUNK_KB (tests): the chunk size.
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

enum { EXIT_ERROR = 2 };

static int die(const char *what) {
    fprintf(stderr, "s5sum: %s (%s)\n", what, s5gpu_last_error());
    return -1;
}
static int rec_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_ZLIB ? S5GPU_REC_ZLIB : m == SLOW5_COMPRESS_ZSTD ? S5GPU_REC_ZSTD : S5GPU_REC_NONE; }
static int sig_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_SVB_ZD ? S5GPU_SIG_SVB_ZD : m == SLOW5_COMPRESS_EX_ZD ? S5GPU_SIG_EX_ZD : S5GPU_SIG_NONE; }

/* ---- XXH64, seed 0 (the published algorithm), for the header text ---- */
static uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static uint64_t le64(const uint8_t *p) { uint64_t v = 0; for (int i = 7; i >= 0; i--) v = (v << 8) | p[i]; return v; }
static uint64_t le32(const uint8_t *p) { return (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24; }
static uint64_t xxh64(const void *data, size_t n) {
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

/* ---- the records of a BLOW5 file, a chunk at a time (s5skim.c): [u64 size][bytes] framed in place, a record the chunk's end cuts carried over ---- */
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
        if (need >= 8) { uint64_t sz; memcpy(&sz, R->buf + R->used, 8); if (sz > 0xFFFFFF00ull) return -1; need = 8 + sz; }
        if (refill(R, need < R->cap ? R->cap : need) != 0) return -1;
        p = R->used;
    }
    if (n == 0 && R->have != R->used) return -1;           /* bytes left over that make no record */
    R->used = p;
    return n;
}

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
static void reader_close(reader_t *R) {
    if (R->buf) s5gpu_host_free(R->buf);
    free(R->rec_pos);
    free(R->rec_len);
}

/* ---- what a file sums to: ids (NUL-terminated, file order) and their digests ---- */
typedef struct {
    char *ids;
    size_t len, cap;
    uint64_t *at, *dig;          /* id i at ids + at[i] */
    uint64_t n, ncap;
    uint64_t header;
} sums_t;

static int sums_add(sums_t *S, const char *id, size_t l, uint64_t dig) {
    if (S->len + l + 1 > S->cap) { S->cap = (S->cap + l + 1) * 2; S->ids = (char *)realloc(S->ids, S->cap); if (!S->ids) return -1; }
    if (S->n + 1 > S->ncap) {
        S->ncap = (S->ncap + 1) * 2;
        S->at = (uint64_t *)realloc(S->at, sizeof(uint64_t) * S->ncap);
        S->dig = (uint64_t *)realloc(S->dig, sizeof(uint64_t) * S->ncap);
        if (!S->at || !S->dig) return -1;
    }
    S->at[S->n] = S->len;
    S->dig[S->n++] = dig;
    memcpy(S->ids + S->len, id, l);
    S->len += l;
    S->ids[S->len++] = '\0';
    return 0;
}
static void sums_free(sums_t *S) { free(S->ids); free(S->at); free(S->dig); }
static uint64_t hash_id(const char *p) {
    uint64_t h = 1469598103934665603ull;
    for (; *p; p++) h = (h ^ (uint8_t)*p) * 1099511628211ull;
    return h;
}
/* the first id that occurs twice, -1: none, -2: out of memory */
static int64_t first_duplicate(const sums_t *S) {
    uint64_t cap = 16;
    while (cap < 2 * S->n) cap *= 2;
    int64_t *tab = (int64_t *)malloc(sizeof(int64_t) * cap);
    if (!tab) return -2;
    for (uint64_t s = 0; s < cap; s++) tab[s] = -1;
    int64_t dup = -1;
    for (uint64_t i = 0; i < S->n && dup < 0; i++) {
        const char *p = S->ids + S->at[i];
        for (uint64_t s = hash_id(p) & (cap - 1);; s = (s + 1) & (cap - 1)) {
            if (tab[s] < 0) { tab[s] = (int64_t)i; break; }
            if (strcmp(S->ids + S->at[tab[s]], p) == 0) { dup = (int64_t)i; break; }
        }
    }
    free(tab);
    return dup;
}

/* --rid's layout of s5skim.c: the aux fields' types only, every role "." — a skim line is only needed for its first column */
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

typedef struct { uint8_t *p; size_t cap; uint64_t *off; } block_t;   /* growable pinned output of a chunk call */

static int report_bad_record(const int32_t *status, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (status[i]) { fprintf(stderr, "s5sum: record %u of the batch is corrupt (status %d)\n", i, status[i]); break; }
    return -1;
}

static int sum_blow5(slow5_file_t *in, const char *path, uint32_t K, size_t chunk, sums_t *S) {
    enum { PITCH = 128 };
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    reader_t R;
    if (reader_open(&R, in, path, K, chunk) != 0) return die("cannot read the records (no end-of-file marker, or out of memory)");
    s5gpu_skim_layout_t *L = NULL;
    block_t o = {NULL, 0, NULL};
    char *ids = (char *)malloc((size_t)K * PITCH);
    uint16_t *id_len = (uint16_t *)malloc(sizeof(uint16_t) * K);
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * K), *dst = (int32_t *)malloc(sizeof(int32_t) * K);
    uint64_t *dig = (uint64_t *)malloc(sizeof(uint64_t) * K);
    if (!ids || !id_len || !st || !dst || !dig) return die("out of memory");
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) return die("damaged record framing");
        if (n == 0) break;
        const int rc = s5gpu_digest_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, sig, dig, dst);
        if (rc == S5GPU_ERR_DATA) return report_bad_record(dst, (uint32_t)n);
        if (rc != S5GPU_OK) return die("digest failed");
        /* the ids: the device id path; zstd records and ids longer than its pitch are the first column of a skim line */
        int need_lines = rec == S5GPU_REC_ZSTD;
        if (!need_lines) {
            if (s5gpu_record_ids_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, PITCH, ids, id_len, st) != S5GPU_OK) return die("read ids failed");
            for (int64_t i = 0; i < n; i++) if (st[i]) need_lines = 1;
        }
        if (need_lines) {
            if (!L) {
                L = (s5gpu_skim_layout_t *)calloc(1, sizeof *L);
                o.cap = (size_t)K * 256 + 4096;
                o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
                o.off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
                if (!L || !o.p || !o.off) return die("out of memory");
                if (rid_layout(in->header->data, in->header->data_len, L) != 0) return die("the header names no column types");
            }
            int src = s5gpu_skim_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, sig, L, o.p, o.cap, o.off, NULL);
            if (src == S5GPU_ERR_NOMEM) {
                const size_t need = (size_t)o.off[0];
                s5gpu_host_free(o.p);
                o.cap = need + need / 4;
                o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
                if (!o.p) return die("out of memory");
                src = s5gpu_skim_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, sig, L, o.p, o.cap, o.off, NULL);
            }
            if (src != S5GPU_OK) return die("read ids failed");
        }
        for (int64_t i = 0; i < n; i++) {
            int rc2;
            if (rec != S5GPU_REC_ZSTD && st[i] == 0) rc2 = sums_add(S, ids + (size_t)i * PITCH, id_len[i], dig[i]);
            else {
                const char *line = (const char *)o.p + o.off[i];
                const char *tab = (const char *)memchr(line, '\t', o.off[i + 1] - o.off[i]);
                rc2 = tab ? sums_add(S, line, (size_t)(tab - line), dig[i]) : -1;
            }
            if (rc2) return die("out of memory");
        }
    }
    reader_close(&R);
    if (o.p) s5gpu_host_free(o.p);
    free(o.off); free(L); free(ids); free(id_len); free(st); free(dst); free(dig);
    return 0;
}

/* SLOW5 ASCII: K lines at a time -> BLOW5 records (none, none) on the device -> back -> s5gpu_digest_batch */
static int sum_slow5(slow5_file_t *in, uint32_t K, size_t chunk, sums_t *S) {
    const struct slow5_aux_meta *am = in->header->aux_meta;
    size_t tcap = chunk;
    uint8_t *txt = (uint8_t *)s5gpu_host_alloc(tcap + 64);
    block_t o = {NULL, 0, NULL};
    o.cap = chunk;
    o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
    o.off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
    uint64_t *line_pos = (uint64_t *)malloc(sizeof(uint64_t) * K), *dig = (uint64_t *)malloc(sizeof(uint64_t) * K);
    uint32_t *line_len = (uint32_t *)malloc(sizeof(uint32_t) * K);
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * K);
    const void **rec = (const void **)malloc(sizeof(void *) * K);
    size_t *rec_len = (size_t *)malloc(sizeof(size_t) * K);
    if (!txt || !o.p || !o.off || !line_pos || !dig || !line_len || !st || !rec || !rec_len) return die("out of memory");
    char *held = NULL;                                     /* a line read but not yet placed: the chunk was full */
    size_t held_len = 0;
    int at_end = 0;
    while (!at_end || held) {
        uint32_t n = 0;
        size_t have = 0;
        while (n < K) {
            if (!held) {
                held = (char *)slow5_get_next_mem(&held_len, in);
                if (!held) {
                    if (slow5_errno != SLOW5_ERR_EOF) { fprintf(stderr, "s5sum: cannot read a record line\n"); return -1; }
                    at_end = 1;
                    break;
                }
            }
            if (held_len > 0xFFFFFF00u) { fprintf(stderr, "s5sum: a record line is too long\n"); return -1; }
            if (have + held_len + 32 > tcap) {
                if (n) break;                              /* this batch is full: the line opens the next one */
                while (have + held_len + 32 > tcap) tcap *= 2;
                s5gpu_host_free(txt);
                txt = (uint8_t *)s5gpu_host_alloc(tcap + 64);
                if (!txt) return die("out of memory");
            }
            memcpy(txt + have, held, held_len);
            line_pos[n] = have;
            line_len[n] = (uint32_t)held_len;
            have += held_len;
            n++;
            free(held);
            held = NULL;
        }
        if (n == 0) break;
        memset(txt + have, 0, 32);
        int rc = s5gpu_ascii_to_blow5_stream(n, txt, have, line_pos, line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                             NULL, 0, o.p, o.cap, o.off, st);
        if (rc == S5GPU_ERR_NOMEM) {
            const size_t need = (size_t)o.off[0];
            s5gpu_host_free(o.p);
            o.cap = need + need / 4;
            o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
            if (!o.p) return die("out of memory");
            rc = s5gpu_ascii_to_blow5_stream(n, txt, have, line_pos, line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                             NULL, 0, o.p, o.cap, o.off, st);
        }
        if (rc != S5GPU_OK) return die("a record line cannot be parsed");
        for (uint32_t i = 0; i < n; i++) { rec[i] = o.p + o.off[i] + 8; rec_len[i] = (size_t)(o.off[i + 1] - o.off[i] - 8); }
        rc = s5gpu_digest_batch(n, rec, rec_len, S5GPU_REC_NONE, S5GPU_SIG_NONE, dig, st);
        if (rc == S5GPU_ERR_DATA) return report_bad_record(st, n);
        if (rc != S5GPU_OK) return die("digest failed");
        for (uint32_t i = 0; i < n; i++) {
            const char *line = (const char *)txt + line_pos[i];
            const char *tab = (const char *)memchr(line, '\t', line_len[i]);
            if (!tab || sums_add(S, line, (size_t)(tab - line), dig[i]) != 0) return die("out of memory, or a line without columns");
        }
    }
    s5gpu_host_free(txt);
    s5gpu_host_free(o.p);
    free(o.off); free(line_pos); free(dig); free(line_len); free(st); free(rec); free(rec_len);
    return 0;
}

static int sum_file(const char *path, uint32_t K, size_t chunk, sums_t *S) {
    memset(S, 0, sizeof *S);
    slow5_file_t *in = slow5_open(path, "r");              /* tells BLOW5 from SLOW5 ASCII by the file's first bytes */
    if (!in) { fprintf(stderr, "s5sum: cannot open %s\n", path); return -1; }
    S->header = xxh64(in->header->data, in->header->data_len);
    const int rc = in->format == SLOW5_FORMAT_BINARY ? sum_blow5(in, path, K, chunk, S) : sum_slow5(in, K, chunk, S);
    slow5_close(in);
    if (rc) return rc;
    const int64_t dup = first_duplicate(S);
    if (dup == -2) return die("out of memory");
    if (dup >= 0) { fprintf(stderr, "s5sum: read id '%s' occurs more than once in %s\n", S->ids + S->at[dup], path); return -1; }
    return 0;
}

static const sums_t *g_sort;
static int by_id(const void *a, const void *b) {
    return strcmp(g_sort->ids + g_sort->at[*(const uint64_t *)a], g_sort->ids + g_sort->at[*(const uint64_t *)b]);
}
static uint64_t *sorted_by_id(const sums_t *S) {
    uint64_t *ix = (uint64_t *)malloc(sizeof(uint64_t) * (S->n ? S->n : 1));
    if (!ix) return NULL;
    for (uint64_t i = 0; i < S->n; i++) ix[i] = i;
    g_sort = S;
    qsort(ix, S->n, sizeof(uint64_t), by_id);
    return ix;
}

int main(int argc, char **argv) {
    int compare = 0;
    long K = 4096;
    const char *path[2] = {NULL, NULL};
    int np = 0, bad = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--compare")) compare = 1;
        else if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (argv[i][0] != '-' && np < 2) path[np++] = argv[i];
        else bad = 1;
    }
    if (bad || np != (compare ? 2 : 1) || K < 1 || K > (1l << 24)) {
        fprintf(stderr, "usage: s5sum [-K batch] file.[b|s]low5\n       s5sum [-K batch] --compare a.[b|s]low5 b.[b|s]low5\n");
        return EXIT_ERROR;
    }
    if (s5gpu_init(0) != S5GPU_OK) { die("no GPU"); return EXIT_ERROR; }
    size_t chunk = (size_t)64 << 20;
    const char *e = getenv("S5SUM_CHUNK_KB");
    if (e && atoi(e) > 0) chunk = (size_t)atoi(e) << 10;
    static char obuf[1 << 20];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
    sums_t A, B;
    if (sum_file(path[0], (uint32_t)K, chunk, &A) != 0) return EXIT_ERROR;
    if (!compare) {
        uint64_t total = 0;
        printf("#s5sum\t1\txxh64\t%016" PRIx64 "\n", A.header);
        for (uint64_t i = 0; i < A.n; i++) { printf("%016" PRIx64 "\t%s\n", A.dig[i], A.ids + A.at[i]); total += A.dig[i]; }
        printf("#total\t%" PRIu64 "\t%016" PRIx64 "\n", A.n, total);
        if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5sum: write failed\n"); return EXIT_ERROR; }
        sums_free(&A);
        return EXIT_SUCCESS;
    }
    if (sum_file(path[1], (uint32_t)K, chunk, &B) != 0) return EXIT_ERROR;
    uint64_t *ia = sorted_by_id(&A), *ib = sorted_by_id(&B);
    if (!ia || !ib) { fprintf(stderr, "s5sum: out of memory\n"); return EXIT_ERROR; }
    if (A.header != B.header) printf("header\t%016" PRIx64 "\t%016" PRIx64 "\n", A.header, B.header);
    uint64_t i = 0, j = 0, same = 0, other = 0;
    while (i < A.n || j < B.n) {
        const char *a = i < A.n ? A.ids + A.at[ia[i]] : NULL, *b = j < B.n ? B.ids + B.at[ib[j]] : NULL;
        const int c = !a ? 1 : !b ? -1 : strcmp(a, b);
        if (c < 0) { printf("only-in-a\t%s\n", a); other++; i++; }
        else if (c > 0) { printf("only-in-b\t%s\n", b); other++; j++; }
        else {
            if (A.dig[ia[i]] == B.dig[ib[j]]) same++;
            else { printf("differs\t%s\t%016" PRIx64 "\t%016" PRIx64 "\n", a, A.dig[ia[i]], B.dig[ib[j]]); other++; }
            i++; j++;
        }
    }
    printf("same\t%" PRIu64 "\n", same);
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5sum: write failed\n"); return EXIT_ERROR; }
    free(ia); free(ib);
    sums_free(&A); sums_free(&B);
    return other ? 1 : EXIT_SUCCESS;
}
