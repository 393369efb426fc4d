/*
 * s5pileup.c — what the reads of a file say about each reference position: the per-position table of their subsequence DTW alignments
 * against a reference squiggle, accumulated on the GPU (k_sdtw, k_sdtw_dirs, k_sdtw_trace, k_pileup; docs/codecs.md §4.18).
 *
 *   s5pileup [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--max-span W] [--min-depth D] ref.txt file.blow5
 *       <ref_pos>\t<ref_level>\t<depth>\t<events>\t<samples>\t<mean>\t<stdv>\t<min>\t<max>\t<mean_cost>     one line per position of depth >= D
 *   ref.txt, S, Q, M, W, the event parameters and the read ids are those of s5align; D defaults to 1.  ref_level is the quantised int16 of
 *   the position; depth the reads whose alignment covers it; events the query events aligned to it and samples their raw samples; mean,
 *   stdv, min and max are over the quantised event levels (mean = sum / events, stdv = sqrt(max(sumsq / events - mean^2, 0))) and mean_cost
 *   is the mean |level - ref_level|, all three as %.6g.  The totals (reads used, skipped, bad; cells; cost) go to stderr as one line.  A
 *   read without a path is skipped, and why goes to stderr as in s5align.
 *   s5pileup --whole [--tile T] [--band B] [--max-events N] ... : the same ten columns from ALL of a read's events (docs/codecs.md §4.22): the
 *   prefix of Q events finds the anchor as above, then up to N events (default 2^20) are aligned in tiles of T rows (default 256) over
 *   windows of B columns (default 512) as in s5extend, and the whole path is added to the table.  --max-span does not count then.
 *   s5pileup --whole --refine [--iters N] [--slope LO,HI] ... : every read is first put into the reference's units by the rounds of
 *   s5extend --refine (docs/codecs.md §4.24; s5gpu_pileup_set_refine), so mean, stdv, min and max are in the reference's units; a read
 *   whose fit is refused is left out and counts as skipped, and how many there were goes to stderr behind the totals.
 *   Exit 0; 1 when a record is corrupt (its read id, or its number in the file when the id cannot be read, goes to stderr; the other reads
 *   are counted); 2 on any other error.
 *
 * One handle (s5gpu_pileup_open, or s5gpu_pileup_open_whole), one s5gpu_pileup_add_batch (or _whole) per K records (default 4096) and one s5gpu_pileup_close: compressed bytes go
 * up; a status per read comes back, and the table once at the end.  The read ids come as in s5map, for the reads that are
 * named on stderr only.
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2, PITCH = 128 };

static int die(const char *what) {
    fprintf(stderr, "s5pileup: %s (%s)\n", what, s5gpu_last_error());
    return EXIT_ERROR;
}
/* a status of the decoder's, not one of map's or align's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
static int rec_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_ZLIB ? S5GPU_REC_ZLIB : m == SLOW5_COMPRESS_ZSTD ? S5GPU_REC_ZSTD : S5GPU_REC_NONE; }
static int sig_code_of(enum slow5_press_method m) { return m == SLOW5_COMPRESS_SVB_ZD ? S5GPU_SIG_SVB_ZD : m == SLOW5_COMPRESS_EX_ZD ? S5GPU_SIG_EX_ZD : S5GPU_SIG_NONE; }

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

/* one number per line; NULL (and a message) when the file cannot be read, holds no number or a line is no number */
static float *read_reference(const char *path, size_t *n_out) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "s5pileup: cannot open %s\n", path); return NULL; }
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
            fprintf(stderr, "s5pileup: %s line %zu is not a number\n", path, line_no);
            free(v); free(line); fclose(f);
            return NULL;
        }
        if (n == cap) { cap *= 2; v = (float *)realloc(v, sizeof(float) * cap); }
        if (v) v[n++] = (float)x;
    }
    free(line);
    fclose(f);
    if (!v) { fprintf(stderr, "s5pileup: out of memory\n"); return NULL; }
    if (n == 0 || n > (1u << 26)) { fprintf(stderr, "s5pileup: %s holds %s\n", path, n ? "too many numbers" : "no number"); free(v); return NULL; }
    *n_out = n;
    return v;
}

int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, wmax = -1, min_depth = 1, tile = -1, band = -1, emax = -1, iters = 2;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, whole = 0, refine = 0;
    const char *ref_path = NULL, *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--max-span") && i + 1 < argc) wmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-depth") && i + 1 < argc) min_depth = atol(argv[++i]);
        else if (!strcmp(argv[i], "--whole")) whole = 1;
        else if (!strcmp(argv[i], "--refine")) refine = 1;
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (!strcmp(argv[i], "--tile") && i + 1 < argc) { tile = atol(argv[++i]); bad |= tile == -1; }
        else if (!strcmp(argv[i], "--band") && i + 1 < argc) { band = atol(argv[++i]); bad |= band == -1; }
        else if (!strcmp(argv[i], "--max-events") && i + 1 < argc) { emax = atol(argv[++i]); bad |= emax == -1; }
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (iters < 1 || iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) {
        fprintf(stderr, "s5pileup: --iters N (1 .. 4), --slope LO,HI (0 < LO <= HI)\n");
        return EXIT_ERROR;
    }
    if (refine && !whole) bad = 1;                                         /* (it belongs to --whole) */
    if (wmax == -1) wmax = 4 * qmax;
    if (!whole && (tile != -1 || band != -1 || emax != -1)) bad = 1;      /* (they belong to --whole) */
    if (tile == -1) tile = 256;
    if (band == -1) band = 512;
    if (emax == -1) emax = 1l << 20;
    if (tile != 64 && tile != 128 && tile != 256 && tile != 512 && tile != 1024) bad = 1;
    if (band < 64 || band > 4096 || band % 64 || emax < qmin || emax > (1l << 20)) bad = 1;
    if (bad || !path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax || wmax < 1 ||
        wmax > (1l << 20) || min_depth < 1 || min_depth > 0xFFFFFFFFl) {
        fprintf(stderr, "usage: s5pileup [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--max-span W (1 .. 2^20)] [--min-depth D (>= 1)] ref.txt file.blow5\n");
        fprintf(stderr, "       s5pileup --whole [--tile T (64, 128, 256, 512, 1024)] [--band B (a multiple of 64 in 64 .. 4096)] [--max-events N (M .. 2^20)] ... : the table of whole reads\n");
        fprintf(stderr, "       s5pileup --whole --refine [--iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)] ... : every read rescaled to the reference's units first\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    size_t R = 0;
    float *levels = read_reference(ref_path, &R);
    if (!levels) return EXIT_ERROR;
    int16_t *ref = (int16_t *)malloc(sizeof(int16_t) * R);
    if (!ref) return die("out of memory");
    if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
    free(levels);
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    slow5_file_t *in = slow5_open(path, "r");
    if (!in) { fprintf(stderr, "s5pileup: cannot open %s\n", path); return EXIT_ERROR; }
    if (in->format != SLOW5_FORMAT_BINARY) { fprintf(stderr, "s5pileup: %s is SLOW5 text: convert it to BLOW5 first\n", path); return EXIT_ERROR; }
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    const s5gpu_event_params_t dna = {3, 6, 1.4, 9.0, 0.2}, rnap = {7, 14, 2.5, 9.0, 1.0};
    const s5gpu_event_params_t *P = rna ? &rnap : &dna;
    static char obuf[1 << 20];
    setvbuf(stdout, obuf, _IOFBF, sizeof obuf);

    void **mem = (void **)calloc((size_t)K, sizeof(void *));
    size_t *len = (size_t *)malloc(sizeof(size_t) * (size_t)K);
    uint64_t *rec_pos = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)K);
    uint32_t *rec_len = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)K);
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K), *ist = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    char *ids = (char *)malloc((size_t)K * PITCH);
    uint16_t *id_len = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)K);
    void **line = (void **)calloc((size_t)K, sizeof(void *));
    size_t *line_len = (size_t *)malloc(sizeof(size_t) * (size_t)K);
    if (!mem || !len || !rec_pos || !rec_len || !st || !ist || !ids || !id_len || !line || !line_len) return die("out of memory");
    size_t chunk_cap = 0;
    uint8_t *acc = (uint8_t *)malloc(s5gpu_pileup_bytes((uint32_t)R));
    uint8_t *chunk = NULL;
    s5gpu_skim_layout_t *L = NULL;
    if (!acc) return die("out of memory");
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    void *pile = whole ? s5gpu_pileup_open_whole(P, &M, &B, 0, ref, (uint32_t)R) : s5gpu_pileup_open(P, &M, (uint32_t)wmax, ref, (uint32_t)R);
    if (!pile) return die("the table cannot be opened");
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)iters};
    if (refine && s5gpu_pileup_set_refine(pile, &RP) != S5GPU_OK) return die("the rounds cannot be turned on");
    uint64_t n_refused = 0;
    int code = EXIT_SUCCESS, at_end = 0;
    uint64_t n_done = 0;
    while (!at_end) {
        uint32_t n = 0;
        size_t bytes = 0;
        while (n < (uint32_t)K) {
            mem[n] = slow5_get_next_mem(&len[n], in);
            if (!mem[n]) {
                if (slow5_errno != SLOW5_ERR_EOF) { fprintf(stderr, "s5pileup: cannot read record %" PRIu64 " of %s\n", n_done + n, path); return EXIT_ERROR; }
                at_end = 1;
                break;
            }
            if (len[n] > 0xFFFFFF00u) { fprintf(stderr, "s5pileup: record %" PRIu64 " is too large\n", n_done + n); return EXIT_ERROR; }
            bytes += 8 + len[n];
            n++;
        }
        if (n == 0) break;
        const int rc = whole ? s5gpu_pileup_add_batch_whole(pile, n, (const void *const *)mem, len, rec, sig, NULL, NULL, st)
                             : s5gpu_pileup_add_batch(pile, n, (const void *const *)mem, len, rec, sig, NULL, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        int named = 0;                                                                                 /* the ids: only where a read is named */
        for (uint32_t i = 0; i < n; i++) named |= st[i] != 0;
        /* the ids: the device id path over the records framed in one buffer; what it leaves (zstd, long ids) is the first column of a skim line */
        for (uint32_t i = 0; i < n; i++) ist[i] = 5;
        if (named && rec != S5GPU_REC_ZSTD) {
            if (bytes + 64 > chunk_cap) {
                if (chunk) s5gpu_host_free(chunk);
                chunk_cap = bytes + bytes / 4 + 64;
                chunk = (uint8_t *)s5gpu_host_alloc(chunk_cap);
                if (!chunk) return die("out of memory");
            }
            size_t p = 0;
            for (uint32_t i = 0; i < n; i++) {
                const uint64_t sz = len[i];
                memcpy(chunk + p, &sz, 8);
                memcpy(chunk + p + 8, mem[i], len[i]);
                rec_pos[i] = p + 8; rec_len[i] = (uint32_t)len[i];
                p += 8 + len[i];
            }
            if (s5gpu_record_ids_stream(n, chunk, p, rec_pos, rec_len, rec, PITCH, ids, id_len, ist) != S5GPU_OK) return die("read ids failed");
        }
        for (uint32_t i = 0; i < n; i++) {
            line[i] = NULL;
            if (st[i] == 0 || ist[i] == 0 || corrupt_status(st[i])) continue;                                        /* (a corrupt record has no skim line either) */
            if (!L) {
                L = (s5gpu_skim_layout_t *)calloc(1, sizeof *L);
                if (!L) return die("out of memory");
                if (rid_layout(in->header->data, in->header->data_len, L) != 0) return die("the header names no column types");
            }
            const void *r1 = mem[i];
            int32_t s1 = 0;
            if (s5gpu_skim_batch(1, &r1, &len[i], rec, sig, L, &line[i], &line_len[i], &s1) != S5GPU_OK || !line[i]) return die("read ids failed");
        }
        for (uint32_t i = 0; i < n; i++) {
            const char *id = NULL;
            size_t idl = 0;
            if (ist[i] == 0) { id = ids + (size_t)i * PITCH; idl = id_len[i]; }
            else if (line[i]) {
                const char *tab = (const char *)memchr(line[i], '\t', line_len[i]);
                id = (const char *)line[i]; idl = tab ? (size_t)(tab - id) : line_len[i];
            }
            if (corrupt_status(st[i])) {
                if (id) fprintf(stderr, "s5pileup: read %.*s is corrupt (status %d)\n", (int)idl, id, st[i]);
                else fprintf(stderr, "s5pileup: record %" PRIu64 " of the file is corrupt (status %d)\n", n_done + i, st[i]);
                code = EXIT_CORRUPT;
            } else if (st[i] == S5GPU_STATUS_FIT_FLAT || st[i] == S5GPU_STATUS_FIT_RANGE) {
                fprintf(stderr, "s5pileup: read %.*s is left out: its fit is refused (%s)\n", (int)idl, id, st[i] == S5GPU_STATUS_FIT_FLAT ? "flat" : "range");
                n_refused++;
            } else if (st[i] != 0) {
                const char *why = st[i] == S5GPU_STATUS_QUERY_SHORT ? "short" : st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                fprintf(stderr, "s5pileup: read %.*s has no path: %s\n", (int)idl, id, why);
            }
            free(line[i]);
            free(mem[i]);
            mem[i] = NULL;
        }
        n_done += n;
    }
    if (s5gpu_pileup_close(pile, acc) != S5GPU_OK) return die("the table cannot be fetched");
    const s5gpu_pile_total_t *T = (const s5gpu_pile_total_t *)acc;
    const s5gpu_pile_col_t *col = (const s5gpu_pile_col_t *)(acc + sizeof *T);
    for (size_t j = 0; j < R; j++) {
        const s5gpu_pile_col_t *c = &col[j];
        if (c->depth < (uint64_t)min_depth) continue;
        const double ne = (double)c->n_events, mean = (double)c->sum_q / ne, var = (double)c->sumsq_q / ne - mean * mean;
        printf("%zu\t%d\t%u\t%u\t%" PRIu64 "\t%.6g\t%.6g\t%d\t%d\t%.6g\n", j, (int)ref[j], c->depth, c->n_events, c->n_samples, mean, sqrt(var > 0.0 ? var : 0.0),
               c->min_q, c->max_q, (double)c->sum_cost / ne);
    }
    fprintf(stderr, "s5pileup: reads used %" PRIu64 ", skipped %" PRIu64 ", bad %" PRIu64 "; cells %" PRIu64 ", cost %" PRIu64 "; %zu positions\n", T->reads_used,
            T->reads_skipped, T->reads_bad, T->cells, T->cost, R);
    if (refine) fprintf(stderr, "s5pileup: reads refused by the fit %" PRIu64 " (they count as skipped)\n", n_refused);
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5pileup: write failed\n"); return EXIT_ERROR; }
    if (chunk) s5gpu_host_free(chunk);
    slow5_close(in);
    free(mem); free(len); free(rec_pos); free(rec_len); free(st); free(ist); free(ids); free(id_len); free(line); free(line_len);
    free(acc); free(L); free(ref);
    return code;
}
