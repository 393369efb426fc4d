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
 * First pass over B: reader_t and idsrc_t of s5tool.h (the chunk reader and the device id path) give a table of (id, offset, length); no .idx is read or written.  Second
 * pass walks A in file order, K records at a time: ids the same way, B's records by pread, and one s5gpu_diff_add_batch per batch: compressed
 * bytes go up, 80 bytes per pair come back, and the accumulator once at the end.
 */
#define _GNU_SOURCE
#define S5TOOL "s5diff"
#define S5TOOL_DIE (-1)
#include <math.h>
#include <unistd.h>

#include "s5tool.h"

enum { EXIT_DIFFER = 1, EXIT_ERROR = 2 };

/* ---- a file's reads: ids (file order), where their records lie, and a hash table over the ids ---- */
typedef struct {
    idlist_t I;
    uint64_t *off;               /* the bytes of read i's record at file offset off[i] */
    uint32_t *rlen;
    uint8_t *paired;
    int64_t *tab;
    uint64_t tcap;
} table_t;

static int table_add(table_t *S, const char *id, size_t l, uint64_t off, uint32_t rlen) {
    const uint64_t had = S->I.ncap;
    if (idlist_add(&S->I, id, l) != 0) return -1;
    if (S->I.ncap != had) {
        S->off = (uint64_t *)realloc(S->off, sizeof(uint64_t) * S->I.ncap);
        S->rlen = (uint32_t *)realloc(S->rlen, sizeof(uint32_t) * S->I.ncap);
        if (!S->off || !S->rlen) return -1;
    }
    S->off[S->I.n - 1] = off;
    S->rlen[S->I.n - 1] = rlen;
    return 0;
}
static void table_free(table_t *S) { free(S->I.ids); free(S->I.at); free(S->off); free(S->rlen); free(S->paired); free(S->tab); }
static int64_t table_find(const table_t *S, const char *id) { return idlist_find(&S->I, S->tab, S->tcap, id); }
/* builds the hash table; an id that occurs twice is an error */
static int index_or_complain(table_t *S, const char *path) {
    S->paired = (uint8_t *)calloc(S->I.n ? S->I.n : 1, 1);
    const int64_t dup = S->paired ? idlist_index(&S->I, &S->tab, &S->tcap) : -2;
    if (dup == -2) { fprintf(stderr, "s5diff: out of memory\n"); return -1; }
    if (dup >= 0) { complain_duplicate(&S->I, dup, path); return -1; }
    return 0;
}

static const table_t *g_sort;
static int by_id(const void *a, const void *b) {
    return strcmp(idlist_id(&g_sort->I, *(const uint64_t *)a), idlist_id(&g_sort->I, *(const uint64_t *)b));
}
/* the unpaired reads of S, sorted by id */
static uint64_t *unpaired_sorted(const table_t *S, uint64_t *count) {
    uint64_t *ix = (uint64_t *)malloc(sizeof(uint64_t) * (S->I.n ? S->I.n : 1));
    if (!ix) return NULL;
    uint64_t k = 0;
    for (uint64_t i = 0; i < S->I.n; i++) if (!S->paired[i]) ix[k++] = i;
    g_sort = S;
    qsort(ix, k, sizeof(uint64_t), by_id);
    *count = k;
    return ix;
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

/* the ids of a batch; a skim call that failed has no wording of its own in idsrc_batch */
static int ids_of_batch(idsrc_t *I, const reader_t *R, uint32_t n) {
    const int rc = idsrc_batch(I, R, n);
    return rc == 0 || rc == -1 ? rc : die("read ids failed (a corrupt record?)");
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
    static const char TEXT_IS[] = "is a SLOW5 text file: convert it to BLOW5 first (text input is not built)";
    slow5_file_t *fa = open_blow5(path[0], TEXT_IS);
    if (!fa) return EXIT_ERROR;
    slow5_file_t *fb = open_blow5(path[1], TEXT_IS);
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
    if (reader_open(&R, fb, path[1], (uint32_t)K, chunk, 1) != 0) { die("cannot read the records of b (no end-of-file marker, or out of memory)"); return EXIT_ERROR; }
    if (idsrc_open(&I, fb, (uint32_t)K) != 0) return EXIT_ERROR;
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) { die("damaged record framing in b"); return EXIT_ERROR; }
        if (n == 0) break;
        if (ids_of_batch(&I, &R, (uint32_t)n) != 0) return EXIT_ERROR;
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
    if (reader_open(&R, fa, path[0], (uint32_t)K, chunk, 1) != 0) { die("cannot read the records of a (no end-of-file marker, or out of memory)"); return EXIT_ERROR; }
    if (idsrc_open(&I, fa, (uint32_t)K) != 0) return EXIT_ERROR;
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
        if (ids_of_batch(&I, &R, (uint32_t)n) != 0) return EXIT_ERROR;
        uint32_t m = 0;
        size_t need = 0;
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            size_t l;
            const char *id = id_of(&I, i, &l);
            if (!id || table_add(&TA, id, l, 0, 0) != 0) { die("out of memory, or a record without an id"); return EXIT_ERROR; }
            const int64_t j = table_find(&TB, idlist_id(&TA.I, TA.I.n - 1));
            if (j < 0 || TB.paired[j]) continue;            /* (an id twice in a: found when a's table is indexed below) */
            TB.paired[j] = 1;
            pa[m] = R.buf + R.rec_pos[i];
            la[m] = R.rec_len[i];
            lb[m] = TB.rlen[j];
            boff[m] = need;
            ida[m] = TA.I.n - 1;
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
                if (sta[k] || stb[k]) { fprintf(stderr, "s5diff: read '%s' is corrupt (status %d in a, %d in b)\n", idlist_id(&TA.I, ida[k]), sta[k], stb[k]); break; }
            return EXIT_ERROR;
        }
        if (rc != S5GPU_OK) { die("diff failed"); return EXIT_ERROR; }
        for (uint32_t k = 0; k < m; k++) {
            const s5gpu_sig_diff_t *r = &rows[k];
            const char *id = idlist_id(&TA.I, ida[k]);
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
    for (uint64_t i = 0; i < TA.I.n; i++) TA.paired[i] = table_find(&TB, idlist_id(&TA.I, i)) >= 0;
    uint64_t ua = 0, ub = 0;
    uint64_t *xa = unpaired_sorted(&TA, &ua), *xb = unpaired_sorted(&TB, &ub);
    if (!xa || !xb) { fprintf(stderr, "s5diff: out of memory\n"); return EXIT_ERROR; }
    for (uint64_t i = 0, j = 0; i < ua || j < ub;) {
        const char *a = i < ua ? idlist_id(&TA.I, xa[i]) : NULL, *b = j < ub ? idlist_id(&TB.I, xb[j]) : NULL;
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
