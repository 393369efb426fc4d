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
 * A BLOW5 file is read in chunks straight into pinned memory and framed in place (reader_t of s5tool.h); at most K records (default 4096) go
 * to one s5gpu_digest_stream call: compressed bytes go up, 8 bytes per read come back.  The read ids come from the device id path as in
 * `s5skim --rid` (idsrc_t of s5tool.h).  A SLOW5 ASCII file (told from BLOW5 by its first bytes) has its lines converted to BLOW5 records
 * with both presses none by s5gpu_ascii_to_blow5_stream, and those go to s5gpu_digest_batch: that path crosses PCIe twice.  The header
 * digest is XXH64 of the header text as BLOW5 stores it (for a .slow5: the ASCII header without its #slow5_version and #num_read_groups
 * lines), made on the host.  The digest resists accidents, not adversaries.  S5SUM_CHUNK_KB (tests): the chunk size.
 */
#define _GNU_SOURCE
#define S5TOOL "s5sum"
#define S5TOOL_DIE (-1)
#include "s5tool.h"

enum { EXIT_ERROR = 2 };

/* ---- what a file sums to: ids (file order) and their digests ---- */
typedef struct {
    idlist_t I;
    uint64_t *dig;               /* of read i */
    uint64_t header;
} sums_t;

static int sums_add(sums_t *S, const char *id, size_t l, uint64_t dig) {
    const uint64_t had = S->I.ncap;
    if (idlist_add(&S->I, id, l) != 0) return -1;
    if (S->I.ncap != had && !(S->dig = (uint64_t *)realloc(S->dig, sizeof(uint64_t) * S->I.ncap))) return -1;
    S->dig[S->I.n - 1] = dig;
    return 0;
}
static void sums_free(sums_t *S) { free(S->I.ids); free(S->I.at); free(S->dig); }

static int report_bad_record(const int32_t *status, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (status[i]) { fprintf(stderr, "s5sum: record %u of the batch is corrupt (status %d)\n", i, status[i]); break; }
    return -1;
}

static int sum_blow5(slow5_file_t *in, const char *path, uint32_t K, size_t chunk, sums_t *S) {
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    reader_t R;
    idsrc_t I;
    if (reader_open(&R, in, path, K, chunk, 1) != 0) return die("cannot read the records (no end-of-file marker, or out of memory)");
    if (idsrc_open(&I, in, K) != 0) return -1;
    int32_t *dst = (int32_t *)malloc(sizeof(int32_t) * K);
    uint64_t *dig = (uint64_t *)malloc(sizeof(uint64_t) * K);
    if (!dst || !dig) return die("out of memory");
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) return die("damaged record framing");
        if (n == 0) break;
        const int rc = s5gpu_digest_stream((uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, sig, dig, dst);
        if (rc == S5GPU_ERR_DATA) return report_bad_record(dst, (uint32_t)n);
        if (rc != S5GPU_OK) return die("digest failed");
        const int irc = idsrc_batch(&I, &R, (uint32_t)n);
        if (irc == -1) return -1;
        if (irc != S5GPU_OK) return die("read ids failed");
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            size_t l;
            const char *id = id_of(&I, i, &l);
            if (!id || sums_add(S, id, l, dig[i]) != 0) return die("out of memory");
        }
    }
    reader_close(&R);
    idsrc_close(&I);
    free(dst); free(dig);
    return 0;
}

typedef struct { uint8_t *p; size_t cap; uint64_t *off; } block_t;   /* growable pinned output of a chunk call */

/* SLOW5 ASCII: K lines at a time -> BLOW5 records (none, none) on the device -> back -> s5gpu_digest_batch */
static int sum_slow5(slow5_file_t *in, uint32_t K, size_t chunk, sums_t *S) {
    const struct slow5_aux_meta *am = in->header->aux_meta;
    textbatch_t T;
    if (textbatch_open(&T, K, chunk, 1) != 0) return -1;
    block_t o = {NULL, 0, NULL};
    o.cap = chunk;
    o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
    o.off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
    uint64_t *dig = (uint64_t *)malloc(sizeof(uint64_t) * K);
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * K);
    const void **rec = (const void **)malloc(sizeof(void *) * K);
    size_t *rec_len = (size_t *)malloc(sizeof(size_t) * K);
    if (!o.p || !o.off || !dig || !st || !rec || !rec_len) return die("out of memory");
    for (;;) {
        const int64_t nl = textbatch_next(&T, in);
        if (nl < 0) return -1;
        if (nl == 0) break;
        const uint32_t n = (uint32_t)nl;
        int rc = s5gpu_ascii_to_blow5_stream(n, T.txt, T.have, T.line_pos, T.line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                             NULL, 0, o.p, o.cap, o.off, st);
        if (rc == S5GPU_ERR_NOMEM) {
            const size_t need = (size_t)o.off[0];
            s5gpu_host_free(o.p);
            o.cap = need + need / 4;
            o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
            if (!o.p) return die("out of memory");
            rc = s5gpu_ascii_to_blow5_stream(n, T.txt, T.have, T.line_pos, T.line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                             NULL, 0, o.p, o.cap, o.off, st);
        }
        if (rc != S5GPU_OK) return die("a record line cannot be parsed");
        for (uint32_t i = 0; i < n; i++) { rec[i] = o.p + o.off[i] + 8; rec_len[i] = (size_t)(o.off[i + 1] - o.off[i] - 8); }
        rc = s5gpu_digest_batch(n, rec, rec_len, S5GPU_REC_NONE, S5GPU_SIG_NONE, dig, st);
        if (rc == S5GPU_ERR_DATA) return report_bad_record(st, n);
        if (rc != S5GPU_OK) return die("digest failed");
        for (uint32_t i = 0; i < n; i++) {
            const char *line = (const char *)T.txt + T.line_pos[i];
            const char *tab = (const char *)memchr(line, '\t', T.line_len[i]);
            if (!tab || sums_add(S, line, (size_t)(tab - line), dig[i]) != 0) return die("out of memory, or a line without columns");
        }
    }
    textbatch_close(&T);
    s5gpu_host_free(o.p);
    free(o.off); free(dig); free(st); free(rec); free(rec_len);
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
    const int64_t dup = idlist_index(&S->I, NULL, NULL);
    if (dup == -2) return die("out of memory");
    if (dup >= 0) { complain_duplicate(&S->I, dup, path); return -1; }
    return 0;
}

static const sums_t *g_sort;
static int by_id(const void *a, const void *b) {
    return strcmp(idlist_id(&g_sort->I, *(const uint64_t *)a), idlist_id(&g_sort->I, *(const uint64_t *)b));
}
static uint64_t *sorted_by_id(const sums_t *S) {
    uint64_t *ix = (uint64_t *)malloc(sizeof(uint64_t) * (S->I.n ? S->I.n : 1));
    if (!ix) return NULL;
    for (uint64_t i = 0; i < S->I.n; i++) ix[i] = i;
    g_sort = S;
    qsort(ix, S->I.n, sizeof(uint64_t), by_id);
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
    big_stdout();
    sums_t A, B;
    if (sum_file(path[0], (uint32_t)K, chunk, &A) != 0) return EXIT_ERROR;
    if (!compare) {
        uint64_t total = 0;
        printf("#s5sum\t1\txxh64\t%016" PRIx64 "\n", A.header);
        for (uint64_t i = 0; i < A.I.n; i++) { printf("%016" PRIx64 "\t%s\n", A.dig[i], idlist_id(&A.I, i)); total += A.dig[i]; }
        printf("#total\t%" PRIu64 "\t%016" PRIx64 "\n", A.I.n, total);
        if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5sum: write failed\n"); return EXIT_ERROR; }
        sums_free(&A);
        return EXIT_SUCCESS;
    }
    if (sum_file(path[1], (uint32_t)K, chunk, &B) != 0) return EXIT_ERROR;
    uint64_t *ia = sorted_by_id(&A), *ib = sorted_by_id(&B);
    if (!ia || !ib) { fprintf(stderr, "s5sum: out of memory\n"); return EXIT_ERROR; }
    if (A.header != B.header) printf("header\t%016" PRIx64 "\t%016" PRIx64 "\n", A.header, B.header);
    uint64_t i = 0, j = 0, same = 0, other = 0;
    while (i < A.I.n || j < B.I.n) {
        const char *a = i < A.I.n ? idlist_id(&A.I, ia[i]) : NULL, *b = j < B.I.n ? idlist_id(&B.I, ib[j]) : NULL;
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
