/*
 * s5refine.c — per-read level rescaling from the path, and a windowed realign (k_path_fit, k_sdtw_win, k_sdtw_trace_win; docs/codecs.md
 * §4.20): a read's query and the reference are normalised apart, so the line r = a q + b is fitted over the cells of the read's first
 * alignment, the query is requantised with it and aligned again in a window around the first hit, --iters times.
 *
 *   s5refine [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--max-span W] [--pad P] [--iters N] [--slope LO,HI] [--per-event]
 *            ref.txt file.blow5
 *       <read_id>\t<events_used>\t<cost>\t<ref_start>\t<ref_end>\t<scale>\t<shift>\t<rounds>\t<cost_refined>\t<ref_start_refined>\t
 *       <ref_end_refined>\t<fit>                                                                  one line per read, reads in file order
 *   ref.txt, S, Q, M, W, the event parameters, the read ids and the exit codes are those of s5align.  cost, ref_start, ref_end: the first
 *   mapping (s5map's columns); scale and shift: a and b of the last round that succeeded as %.9g (1 and 0: none did); rounds: how many did;
 *   the refined columns: the row of that round (the first mapping's when none did); fit: `ok`, or why the rounds ended early: `flat` (too
 *   few cells or a query without variance along the path), `range` (a slope outside LO,HI, default 0.5,2, or a shift above 64), `wide` (the
 *   window [start - P, end + P] is above W).  P defaults to 16, N to 2 (1 .. 4).  A read without a path prints `*` in every column behind
 *   its id, and why goes to stderr as in s5align.
 *   --per-event: the lines of s5align instead, made from the refined path (the first path where no round succeeded).
 *
 * At most K records (default 4096) go to one s5gpu_refine_batch call: compressed bytes go up; both rows, the fit, the refined lo and hi and
 * the query's event rows come back in one download.  The read ids come from batch_ids of s5tool.h.
 */
#define _GNU_SOURCE
#define S5TOOL "s5refine"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's, align's or refine's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, wmax = -1, pad = 16, iters = 2;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, per_event = 0;
    const char *ref_path = NULL, *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--max-span") && i + 1 < argc) wmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--pad") && i + 1 < argc) pad = atol(argv[++i]);
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (!strcmp(argv[i], "--per-event")) per_event = 1;
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (wmax == -1) wmax = 4 * qmax;
    if (bad || !path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax || wmax < 1 ||
        wmax > (1l << 20) || pad < 0 || pad > 65535 || iters < 1 || iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) {
        fprintf(stderr, "usage: s5refine [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--max-span W (1 .. 2^20)] "
                        "[--pad P (0 .. 65535)] [--iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)] [--per-event] ref.txt file.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, (uint32_t)pad, 16, (uint32_t)iters};
    size_t R = 0;
    float *levels = read_reference(ref_path, 0x7FFFFFFFu, "too many numbers", &R);
    if (!levels) return EXIT_ERROR;
    int16_t *ref = (int16_t *)malloc(sizeof(int16_t) * R);
    if (!ref) return die("out of memory");
    if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
    free(levels);
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    const s5gpu_event_params_t *P = event_params(rna);
    big_stdout();

    batch_t bt;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    if (!st) return die("out of memory");
    s5gpu_map_row_t *rows = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K), *rows2 = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K);
    s5gpu_fit_t *fit = (s5gpu_fit_t *)malloc(sizeof(s5gpu_fit_t) * (size_t)K);
    uint32_t *rounds = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)K);
    int32_t *lo = (int32_t *)malloc(sizeof(int32_t) * (size_t)K * (size_t)qmax), *hi = (int32_t *)malloc(sizeof(int32_t) * (size_t)K * (size_t)qmax);
    s5gpu_event_t *ev = (s5gpu_event_t *)malloc(sizeof(s5gpu_event_t) * (size_t)K * (size_t)qmax);
    if (!rows || !rows2 || !fit || !rounds || !lo || !hi || !ev) return die("out of memory");
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = s5gpu_refine_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, (uint32_t)wmax, &RP, ref, (uint32_t)R, rows, rows2, fit, lo, hi, ev,
                                          st, rounds);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("refinement failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < n; i++) {
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            if (corrupt_status(st[i])) {
                batch_corrupt(&bt, i, st[i]);
                code = EXIT_CORRUPT;
            } else if (st[i] == S5GPU_STATUS_QUERY_SHORT || rows2[i].qlen == 0) {                        /* no path: short, or wide / row before any round */
                const char *why = st[i] == S5GPU_STATUS_QUERY_SHORT ? "short" : st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                fprintf(stderr, "s5refine: read %.*s has no path: %s\n", (int)idl, id, why);
                if (per_event) printf("%.*s\t*\t*\t*\t*\t*\t*\n", (int)idl, id);
                else printf("%.*s\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\n", (int)idl, id);
            } else if (per_event) {
                const size_t at = (size_t)i * (size_t)qmax;
                for (uint32_t k = 0; k < rows2[i].qlen; k++) {
                    const s5gpu_event_t *e = &ev[at + k];
                    printf("%.*s\t%" PRIu64 "\t%u\t%" PRIu64 "\t%.6g\t%d\t%d\n", (int)idl, id, (uint64_t)skip + k, e->start, (uint64_t)e->start + e->length,
                           (double)e->mean, lo[at + k], hi[at + k]);
                }
            } else {
                const char *how = st[i] == 0 ? "ok" : st[i] == S5GPU_STATUS_FIT_FLAT ? "flat" : st[i] == S5GPU_STATUS_FIT_RANGE ? "range" :
                                  st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                printf("%.*s\t%u\t%u\t%d\t%d\t%.9g\t%.9g\t%u\t%u\t%d\t%d\t%s\n", (int)idl, id, rows[i].qlen, rows[i].cost, rows[i].start, rows[i].end, fit[i].a,
                       fit[i].b, rounds[i], rows2[i].cost, rows2[i].start, rows2[i].end, how);
            }
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5refine: write failed\n"); return EXIT_ERROR; }
    batch_close(&bt);
    slow5_close(in);
    free(st);
    free(rows); free(rows2); free(fit); free(rounds); free(lo); free(hi); free(ev); free(ref);
    return code;
}
