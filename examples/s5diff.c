/*
 * s5diff.c — where and by how much do the reads of two BLOW5 files differ?  The reads are paired by id and compared where the decoder left
 * them on the GPU (k_sig_diff, docs/codecs.md §4.14): signal error per read and file-wide, field, aux and length differences.  The result
 * does not depend on the presses of either file or on the order of the reads.
 *
 *   s5diff [-K batch] [--tol T] [--hist FILE] a.blow5 b.blow5
 *       #s5diff\t1
 *       header\t<digest a>\t<digest b>         when the header digests of s5sum differ (does not change the exit code)
 *       aux-layout                             when the aux name / type lines of the headers differ: AUX flags are then masked out and not counted
 *       <read_id>\t<flag names joined by ','>\t<n_a>\t<n_b>\t<n_diff>\t<first_diff>\t<max_abs>\t<max_at>\t<rmse>
 *                                              one line per pair whose flags are not 0, in A's order; rmse = sqrt(sum_sq / n_cmp) as %.6g;
 *                                              "-" for an index that does not exist and for the rmse of n_cmp == 0
 *       only-in-a\t<id> | only-in-b\t<id>      sorted by id (one sorted sequence, as s5sum --compare prints them)
 *       #pairs\t<n>\t<n_differ>   #samples\t<n_samples>\t<n_diff>   #max_abs   #sum_abs   #sum_sq   #rmse (%.6g, "-" without samples)
 *       #snr_db                                10 log10(sumsq_a / sum_sq) as %.4f; "inf" when sum_sq == 0
 *       --hist FILE: `d <tab> count` for every difference d that occurs, in order of d.
 *   Exit 0: no flagged pair and no unpaired id; 1 otherwise; 2: any error (unreadable or damaged file, corrupt record, an id that occurs twice
 *   in one file, a .slow5 argument: text input is not built, convert it first).  With --tol T exit 0 also when every flagged pair has flags
 *   exactly `signal` and max_abs <= T, and no id is unpaired.
 *
 * First pass over B: the reader of s5sum.c and the device id path give a table of (id, offset, length); no .idx is read or written.  Second
 * pass walks A in file order, K records at a time: ids the same way, B's records by pread, and one s5gpu_diff_add_batch per batch: compressed
 * bytes go up, 80 bytes per pair come back, and the accumulator once at the end.
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

enum { EXIT_DIFFER = 1, EXIT_ERROR = 2, PITCH = 128 };

static int die(const char *what) {
    fprintf(stderr, "s5diff: %s (%s)\n", what, s5gpu_last_error());
    return -1;
}
static int rec_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_ZLIB ? S5GPU_REC_ZLIB : m == SLOW5_COMPRESS_ZSTD ? S5GPU_REC_ZSTD : S5GPU_REC_NONE; }
static int sig_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_SVB_ZD ? S5GPU_SIG_SVB_ZD : m == SLOW5_COMPRESS_EX_ZD ? S5GPU_SIG_EX_ZD : S5GPU_SIG_NONE; }

/* ---- XXH64, seed 0 (the published algorithm), for the header text: the header digest of s5sum ---- */
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

/* ---- the records of a BLOW5 file, a chunk at a time (s5sum.c): [u64 size][bytes] framed in place, a record the chunk's end cuts carried over ---- */
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
        size_t need = R->have - R->used;
        if (need >= 8) { uint64_t sz; memcpy(&sz, R->buf + R->used, 8); if (sz > 0xFFFFFF00ull) return -1; need = 8 + sz; }
        if (refill(R, need < R->cap ? R->cap : need) != 0) return -1;
        p = R->used;
    }
    if (n == 0 && R->have != R->used) return -1;           /* bytes left over that make no record */
    R->used = p;
    return n;
}
/* the file offset of the byte at buffer offset p */
static uint64_t file_offset(const reader_t *R, uint64_t p) { return R->pos - R->have + p; }

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

/* ---- the ids of a batch: the device id path; zstd records and ids longer than its pitch are the first column of a skim line (s5sum.c) ---- */
typedef struct {
    slow5_file_t *in;
    int rec, sig;
    uint32_t K;
    char *ids;
    uint16_t *id_len;
    int32_t *st;
    s5gpu_skim_layout_t *L;
    uint8_t *txt;
    size_t txt_cap;
    uint64_t *txt_off;
} idsrc_t;

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
static int idsrc_open(idsrc_t *I, slow5_file_t *in, uint32_t K) {
    memset(I, 0, sizeof *I);
    I->in = in;
    I->rec = rec_code_of(in->compress->record_press->method);
    I->sig = sig_code_of(in->compress->signal_press->method);
    I->K = K;
    I->ids = (char *)malloc((size_t)K * PITCH);
    I->id_len = (uint16_t *)malloc(sizeof(uint16_t) * K);
    I->st = (int32_t *)malloc(sizeof(int32_t) * K);
    return I->ids && I->id_len && I->st ? 0 : -1;
}
static void idsrc_close(idsrc_t *I) {
    if (I->txt) s5gpu_host_free(I->txt);
    free(I->ids); free(I->id_len); free(I->st); free(I->L); free(I->txt_off);
}
/* the ids of the n records the reader has framed; afterwards id_of(I, i, &len) */
static int idsrc_batch(idsrc_t *I, const reader_t *R, uint32_t n) {
    int need_lines = I->rec == S5GPU_REC_ZSTD;
    if (!need_lines) {
        if (s5gpu_record_ids_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, I->rec, PITCH, I->ids, I->id_len, I->st) != S5GPU_OK) return die("read ids failed");
        for (uint32_t i = 0; i < n; i++) if (I->st[i]) need_lines = 1;
    } else for (uint32_t i = 0; i < n; i++) I->st[i] = 1;
    if (!need_lines) return 0;
    if (!I->L) {
        I->L = (s5gpu_skim_layout_t *)calloc(1, sizeof *I->L);
        I->txt_cap = (size_t)I->K * 256 + 4096;
        I->txt = (uint8_t *)s5gpu_host_alloc(I->txt_cap);
        I->txt_off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)I->K + 1));
        if (!I->L || !I->txt || !I->txt_off) return die("out of memory");
        if (rid_layout(I->in->header->data, I->in->header->data_len, I->L) != 0) return die("the header names no column types");
    }
    int rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, I->rec, I->sig, I->L, I->txt, I->txt_cap, I->txt_off, NULL);
    if (rc == S5GPU_ERR_NOMEM) {
        const size_t need = (size_t)I->txt_off[0];
        s5gpu_host_free(I->txt);
        I->txt_cap = need + need / 4;
        I->txt = (uint8_t *)s5gpu_host_alloc(I->txt_cap);
        if (!I->txt) return die("out of memory");
        rc = s5gpu_skim_stream(n, R->buf, R->have, R->rec_pos, R->rec_len, I->rec, I->sig, I->L, I->txt, I->txt_cap, I->txt_off, NULL);
    }
    return rc == S5GPU_OK ? 0 : die("read ids failed (a corrupt record?)");
}
static const char *id_of(const idsrc_t *I, uint32_t i, size_t *len) {
    if (I->st[i] == 0) { *len = I->id_len[i]; return I->ids + (size_t)i * PITCH; }
    const char *line = (const char *)I->txt + I->txt_off[i];
    const char *tab = (const char *)memchr(line, '\t', I->txt_off[i + 1] - I->txt_off[i]);
    *len = tab ? (size_t)(tab - line) : 0;
    return tab ? line : NULL;
}

/* ---- a file's reads: ids (NUL-terminated, file order), where their records lie, and a hash table over the ids ---- */
typedef struct {
    char *ids;
    size_t len, cap;
    uint64_t *at, *off;          /* id i at ids + at[i]; its record's bytes at file offset off[i] */
    uint32_t *rlen;
    uint8_t *paired;
    uint64_t n, ncap;
    int64_t *tab;
    uint64_t tcap;
} table_t;

static int table_add(table_t *S, const char *id, size_t l, uint64_t off, uint32_t rlen) {
    if (S->len + l + 1 > S->cap) { S->cap = (S->cap + l + 1) * 2; S->ids = (char *)realloc(S->ids, S->cap); if (!S->ids) return -1; }
    if (S->n + 1 > S->ncap) {
        S->ncap = (S->ncap + 1) * 2;
        S->at = (uint64_t *)realloc(S->at, sizeof(uint64_t) * S->ncap);
        S->off = (uint64_t *)realloc(S->off, sizeof(uint64_t) * S->ncap);
        S->rlen = (uint32_t *)realloc(S->rlen, sizeof(uint32_t) * S->ncap);
        if (!S->at || !S->off || !S->rlen) return -1;
    }
    S->at[S->n] = S->len;
    S->off[S->n] = off;
    S->rlen[S->n++] = rlen;
    memcpy(S->ids + S->len, id, l);
    S->len += l;
    S->ids[S->len++] = '\0';
    return 0;
}
static void table_free(table_t *S) { free(S->ids); free(S->at); free(S->off); free(S->rlen); free(S->paired); free(S->tab); }
static uint64_t hash_id(const char *p) {
    uint64_t h = 1469598103934665603ull;
    for (; *p; p++) h = (h ^ (uint8_t)*p) * 1099511628211ull;
    return h;
}
/* builds the hash table; the first id that occurs twice, -1: none, -2: out of memory */
static int64_t table_index(table_t *S) {
    S->tcap = 16;
    while (S->tcap < 2 * S->n) S->tcap *= 2;
    S->tab = (int64_t *)malloc(sizeof(int64_t) * S->tcap);
    S->paired = (uint8_t *)calloc(S->n ? S->n : 1, 1);
    if (!S->tab || !S->paired) return -2;
    for (uint64_t s = 0; s < S->tcap; s++) S->tab[s] = -1;
    for (uint64_t i = 0; i < S->n; i++) {
        const char *p = S->ids + S->at[i];
        for (uint64_t s = hash_id(p) & (S->tcap - 1);; s = (s + 1) & (S->tcap - 1)) {
            if (S->tab[s] < 0) { S->tab[s] = (int64_t)i; break; }
            if (strcmp(S->ids + S->at[S->tab[s]], p) == 0) return (int64_t)i;
        }
    }
    return -1;
}
static int64_t table_find(const table_t *S, const char *id) {   /* id NUL-terminated */
    for (uint64_t s = hash_id(id) & (S->tcap - 1);; s = (s + 1) & (S->tcap - 1)) {
        if (S->tab[s] < 0) return -1;
        if (strcmp(S->ids + S->at[S->tab[s]], id) == 0) return S->tab[s];
    }
}
static int index_or_complain(table_t *S, const char *path) {
    const int64_t dup = table_index(S);
    if (dup == -2) { fprintf(stderr, "s5diff: out of memory\n"); return -1; }
    if (dup >= 0) { fprintf(stderr, "s5diff: read id '%s' occurs more than once in %s\n", S->ids + S->at[dup], path); return -1; }
    return 0;
}

static const table_t *g_sort;
static int by_id(const void *a, const void *b) {
    return strcmp(g_sort->ids + g_sort->at[*(const uint64_t *)a], g_sort->ids + g_sort->at[*(const uint64_t *)b]);
}
/* the unpaired reads of S, sorted by id */
static uint64_t *unpaired_sorted(const table_t *S, uint64_t *count) {
    uint64_t *ix = (uint64_t *)malloc(sizeof(uint64_t) * (S->n ? S->n : 1));
    if (!ix) return NULL;
    uint64_t k = 0;
    for (uint64_t i = 0; i < S->n; i++) if (!S->paired[i]) ix[k++] = i;
    g_sort = S;
    qsort(ix, k, sizeof(uint64_t), by_id);
    *count = k;
    return ix;
}

static slow5_file_t *open_blow5(const char *path) {
    slow5_file_t *in = slow5_open(path, "r");              /* tells BLOW5 from SLOW5 ASCII by the file's first bytes */
    if (!in) { fprintf(stderr, "s5diff: cannot open %s\n", path); return NULL; }
    if (in->format != SLOW5_FORMAT_BINARY) {
        fprintf(stderr, "s5diff: %s is a SLOW5 text file: convert it to BLOW5 first (text input is not built)\n", path);
        slow5_close(in);
        return NULL;
    }
    return in;
}

/* the line of the header text that starts with `prefix` */
static const char *header_line(const char *h, size_t len, const char *prefix, size_t *l_out) {
    const size_t pl = strlen(prefix);
    size_t b = 0;
    while (b < len) {
        const char *e = (const char *)memchr(h + b, '\n', len - b);
        const size_t l = e ? (size_t)(e - h) - b : len - b;
        if (l >= pl && memcmp(h + b, prefix, pl) == 0) { *l_out = l; return h + b; }
        b += l + 1;
    }
    *l_out = 0;
    return NULL;
}
static int same_line(slow5_file_t *a, slow5_file_t *b, const char *prefix) {
    size_t la, lb;
    const char *pa = header_line(a->header->data, a->header->data_len, prefix, &la), *pb = header_line(b->header->data, b->header->data_len, prefix, &lb);
    return (!pa && !pb) || (pa && pb && la == lb && memcmp(pa, pb, la) == 0);
}

static const char *const FLAG_NAME[9] = {"signal", "len", "read_group", "digitisation", "offset", "range", "sampling_rate", "id", "aux"};

static void print_index(FILE *o, uint32_t v) {
    if (v == S5GPU_DIFF_NONE) fputs("\t-", o);
    else fprintf(o, "\t%" PRIu32, v);
}

int main(int argc, char **argv) {
    long K = 4096, tol = -1;
    const char *path[2] = {NULL, NULL}, *hist_path = NULL;
    int np = 0, bad = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--tol") && i + 1 < argc) { char *e; tol = strtol(argv[++i], &e, 10); if (*e || tol < 0) bad = 1; }
        else if (!strcmp(argv[i], "--hist") && i + 1 < argc) hist_path = argv[++i];
        else if (argv[i][0] != '-' && np < 2) path[np++] = argv[i];
        else bad = 1;
    }
    if (bad || np != 2 || K < 1 || K > (1l << 24)) {
        fprintf(stderr, "usage: s5diff [-K batch] [--tol T] [--hist FILE] a.blow5 b.blow5\n");
        return EXIT_ERROR;
    }
    slow5_file_t *fa = open_blow5(path[0]);
    if (!fa) return EXIT_ERROR;
    slow5_file_t *fb = open_blow5(path[1]);
    if (!fb) return EXIT_ERROR;
    if (s5gpu_init(0) != S5GPU_OK) { die("no GPU"); return EXIT_ERROR; }
    const size_t chunk = (size_t)64 << 20;

    char *text = NULL;                                     /* everything is printed at the end: an error leaves stdout empty */
    size_t text_len = 0;
    FILE *o = open_memstream(&text, &text_len);
    if (!o) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
    fprintf(o, "#s5diff\t1\n");
    const uint64_t ha = xxh64(fa->header->data, fa->header->data_len), hb = xxh64(fb->header->data, fb->header->data_len);
    if (ha != hb) fprintf(o, "header\t%016" PRIx64 "\t%016" PRIx64 "\n", ha, hb);
    const int aux_layout = !same_line(fa, fb, "#char*") || !same_line(fa, fb, "#read_id");
    if (aux_layout) fprintf(o, "aux-layout\n");
    const uint32_t mask = aux_layout ? ~(uint32_t)S5GPU_DIFF_AUX : ~0u;

    /* pass 1: B's table */
    table_t TB, TA;
    memset(&TB, 0, sizeof TB);
    memset(&TA, 0, sizeof TA);
    reader_t R;
    idsrc_t I;
    if (reader_open(&R, fb, path[1], (uint32_t)K, chunk) != 0) { die("cannot read the records of b (no end-of-file marker, or out of memory)"); return EXIT_ERROR; }
    if (idsrc_open(&I, fb, (uint32_t)K) != 0) { die("out of memory"); return EXIT_ERROR; }
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) { die("damaged record framing in b"); return EXIT_ERROR; }
        if (n == 0) break;
        if (idsrc_batch(&I, &R, (uint32_t)n) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            size_t l;
            const char *id = id_of(&I, i, &l);
            if (!id || table_add(&TB, id, l, file_offset(&R, R.rec_pos[i]), R.rec_len[i]) != 0) { die("out of memory, or a record without an id"); return EXIT_ERROR; }
        }
    }
    reader_close(&R);
    idsrc_close(&I);
    if (index_or_complain(&TB, path[1]) != 0) return EXIT_ERROR;

    /* pass 2: A in file order */
    void *h = s5gpu_diff_open();
    if (!h) { die("no diff handle"); return EXIT_ERROR; }
    if (reader_open(&R, fa, path[0], (uint32_t)K, chunk) != 0) { die("cannot read the records of a (no end-of-file marker, or out of memory)"); return EXIT_ERROR; }
    if (idsrc_open(&I, fa, (uint32_t)K) != 0) { die("out of memory"); return EXIT_ERROR; }
    const int rec_a = I.rec, sig_a = I.sig, rec_b = rec_code_of(fb->compress->record_press->method), sig_b = sig_code_of(fb->compress->signal_press->method);
    const void **pa = (const void **)malloc(sizeof(void *) * (size_t)K), **pb = (const void **)malloc(sizeof(void *) * (size_t)K);
    size_t *la = (size_t *)malloc(sizeof(size_t) * (size_t)K), *lb = (size_t *)malloc(sizeof(size_t) * (size_t)K);
    uint64_t *ida = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)K), *boff = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)K);
    s5gpu_sig_diff_t *rows = (s5gpu_sig_diff_t *)malloc(sizeof(s5gpu_sig_diff_t) * (size_t)K);
    int32_t *sta = (int32_t *)malloc(sizeof(int32_t) * (size_t)K), *stb = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    uint8_t *bbuf = NULL;
    size_t bcap = 0;
    if (!pa || !pb || !la || !lb || !ida || !boff || !rows || !sta || !stb) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
    const int fdb = fileno(fb->fp);
    uint64_t n_pairs = 0, n_differ = 0, out_of_tol = 0;
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) { die("damaged record framing in a"); return EXIT_ERROR; }
        if (n == 0) break;
        if (idsrc_batch(&I, &R, (uint32_t)n) != 0) return EXIT_ERROR;
        uint32_t m = 0;
        size_t need = 0;
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            size_t l;
            const char *id = id_of(&I, i, &l);
            if (!id || table_add(&TA, id, l, 0, 0) != 0) { die("out of memory, or a record without an id"); return EXIT_ERROR; }
            const int64_t j = table_find(&TB, TA.ids + TA.at[TA.n - 1]);
            if (j < 0 || TB.paired[j]) continue;            /* (an id twice in a: found when a's table is indexed below) */
            TB.paired[j] = 1;
            pa[m] = R.buf + R.rec_pos[i];
            la[m] = R.rec_len[i];
            lb[m] = TB.rlen[j];
            boff[m] = need;
            ida[m] = TA.n - 1;
            need += ((size_t)TB.rlen[j] + 15) & ~(size_t)15;
            /* the offset in b's file rides in pb until the buffer is known */
            pb[m] = (const void *)(uintptr_t)TB.off[j];
            m++;
        }
        if (need + 64 > bcap) {
            free(bbuf);
            bcap = need + need / 4 + 4096;
            bbuf = (uint8_t *)malloc(bcap);
            if (!bbuf) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
        }
        for (uint32_t k = 0; k < m; k++) {
            const uint64_t off = (uint64_t)(uintptr_t)pb[k];
            if (pread(fdb, bbuf + boff[k], lb[k], (off_t)off) != (ssize_t)lb[k]) { fprintf(stderr, "s5diff: cannot read a record of %s\n", path[1]); return EXIT_ERROR; }
            pb[k] = bbuf + boff[k];
        }
        if (m == 0) continue;
        const int rc = s5gpu_diff_add_batch(h, m, pa, la, rec_a, sig_a, pb, lb, rec_b, sig_b, rows, sta, stb);
        if (rc == S5GPU_ERR_DATA) {
            for (uint32_t k = 0; k < m; k++)
                if (sta[k] || stb[k]) { fprintf(stderr, "s5diff: read '%s' is corrupt (status %d in a, %d in b)\n", TA.ids + TA.at[ida[k]], sta[k], stb[k]); break; }
            return EXIT_ERROR;
        }
        if (rc != S5GPU_OK) { die("diff failed"); return EXIT_ERROR; }
        for (uint32_t k = 0; k < m; k++) {
            const s5gpu_sig_diff_t *r = &rows[k];
            const char *id = TA.ids + TA.at[ida[k]];
            if (r->flags & (S5GPU_DIFF_FAILED | S5GPU_DIFF_BAD_PAIR)) { fprintf(stderr, "s5diff: read '%s' cannot be compared (its fields point outside its record)\n", id); return EXIT_ERROR; }
            const uint32_t fl = r->flags & mask;
            n_pairs++;
            if (!fl) continue;
            n_differ++;
            if (fl != S5GPU_DIFF_SIGNAL || (tol >= 0 && r->max_abs > (uint64_t)tol)) out_of_tol++;
            fprintf(o, "%s\t", id);
            int first = 1;
            for (int b = 0; b < 9; b++)
                if (fl >> b & 1) { fprintf(o, "%s%s", first ? "" : ",", FLAG_NAME[b]); first = 0; }
            fprintf(o, "\t%" PRIu32 "\t%" PRIu32 "\t%" PRIu32, r->n_a, r->n_b, r->n_diff);
            print_index(o, r->first_diff);
            fprintf(o, "\t%" PRIu32, r->max_abs);
            print_index(o, r->max_at);
            const uint32_t n_cmp = r->n_a < r->n_b ? r->n_a : r->n_b;
            if (n_cmp) fprintf(o, "\t%.6g\n", sqrt((double)r->sum_sq / (double)n_cmp));
            else fputs("\t-\n", o);
        }
    }
    reader_close(&R);
    idsrc_close(&I);
    if (index_or_complain(&TA, path[0]) != 0) return EXIT_ERROR;
    s5gpu_diff_acc_t *acc = (s5gpu_diff_acc_t *)malloc(sizeof *acc);
    if (!acc) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
    if (s5gpu_diff_close(h, acc) != S5GPU_OK) { die("the accumulator did not come back"); return EXIT_ERROR; }

    /* the unpaired ids of both files as one sorted sequence */
    for (uint64_t i = 0; i < TA.n; i++) TA.paired[i] = table_find(&TB, TA.ids + TA.at[i]) >= 0;
    uint64_t ua = 0, ub = 0;
    uint64_t *xa = unpaired_sorted(&TA, &ua), *xb = unpaired_sorted(&TB, &ub);
    if (!xa || !xb) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
    for (uint64_t i = 0, j = 0; i < ua || j < ub;) {
        const char *a = i < ua ? TA.ids + TA.at[xa[i]] : NULL, *b = j < ub ? TB.ids + TB.at[xb[j]] : NULL;
        if (a && (!b || strcmp(a, b) < 0)) { fprintf(o, "only-in-a\t%s\n", a); i++; }
        else { fprintf(o, "only-in-b\t%s\n", b); j++; }
    }
    fprintf(o, "#pairs\t%" PRIu64 "\t%" PRIu64 "\n", n_pairs, n_differ);
    fprintf(o, "#samples\t%" PRIu64 "\t%" PRIu64 "\n", acc->n_samples, acc->n_diff);
    fprintf(o, "#max_abs\t%" PRIu32 "\n#sum_abs\t%" PRIu64 "\n#sum_sq\t%" PRIu64 "\n", acc->max_abs, acc->sum_abs, acc->sum_sq);
    if (acc->n_samples) fprintf(o, "#rmse\t%.6g\n", sqrt((double)acc->sum_sq / (double)acc->n_samples));
    else fprintf(o, "#rmse\t-\n");
    if (acc->sum_sq == 0) fprintf(o, "#snr_db\tinf\n");
    else fprintf(o, "#snr_db\t%.4f\n", 10.0 * log10((double)acc->sumsq_a / (double)acc->sum_sq));
    if (hist_path) {
        FILE *hf = fopen(hist_path, "w");
        if (!hf) { fprintf(stderr, "s5diff: cannot write %s\n", hist_path); return EXIT_ERROR; }
        for (int64_t b = 0; b < S5GPU_DIFF_BINS; b++)
            if (acc->hist[b]) fprintf(hf, "%" PRId64 "\t%" PRIu64 "\n", b - 65535, acc->hist[b]);
        if (fclose(hf) != 0) { fprintf(stderr, "s5diff: write failed\n"); return EXIT_ERROR; }
    }
    if (fclose(o) != 0 || fwrite(text, 1, text_len, stdout) != text_len || fflush(stdout) != 0) { fprintf(stderr, "s5diff: write failed\n"); return EXIT_ERROR; }
    free(text); free(acc); free(xa); free(xb); free(pa); free(pb); free(la); free(lb); free(ida); free(boff); free(rows); free(sta); free(stb); free(bbuf);
    table_free(&TA); table_free(&TB);
    slow5_close(fa); slow5_close(fb);
    const int clean = n_differ == 0 || (tol >= 0 && out_of_tol == 0);
    return clean && ua == 0 && ub == 0 ? EXIT_SUCCESS : EXIT_DIFFER;
}
