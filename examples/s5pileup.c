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
 * up; a status per read comes back, and the table once at the end.  The read ids come from batch_ids of s5tool.h, for the reads that
 * are named on stderr only.
 */
#define _GNU_SOURCE
#define S5TOOL "s5pileup"
#define S5TOOL_DIE 2
#include <math.h>

#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's or align's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
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
    float *levels = read_reference(ref_path, (1u << 26), "too many numbers", &R);
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
    uint8_t *acc = (uint8_t *)malloc(s5gpu_pileup_bytes((uint32_t)R));
    if (!acc) return die("out of memory");
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    void *pile = whole ? s5gpu_pileup_open_whole(P, &M, &B, 0, ref, (uint32_t)R) : s5gpu_pileup_open(P, &M, (uint32_t)wmax, ref, (uint32_t)R);
    if (!pile) return die("the table cannot be opened");
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)iters};
    if (refine && s5gpu_pileup_set_refine(pile, &RP) != S5GPU_OK) return die("the rounds cannot be turned on");
    uint64_t n_refused = 0;
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = whole ? s5gpu_pileup_add_batch_whole(pile, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, NULL, NULL, st)
                             : s5gpu_pileup_add_batch(pile, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, NULL, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        if (batch_ids(&bt, st, corrupt_status, 1) != 0) return EXIT_ERROR;                    /* the ids: only where a read is named */
        for (uint32_t i = 0; i < n; i++) {
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            if (corrupt_status(st[i])) {
                batch_corrupt(&bt, i, st[i]);
                code = EXIT_CORRUPT;
            } else if (st[i] == S5GPU_STATUS_FIT_FLAT || st[i] == S5GPU_STATUS_FIT_RANGE) {
                fprintf(stderr, "s5pileup: read %.*s is left out: its fit is refused (%s)\n", (int)idl, id, st[i] == S5GPU_STATUS_FIT_FLAT ? "flat" : "range");
                n_refused++;
            } else if (st[i] != 0) {
                const char *why = st[i] == S5GPU_STATUS_QUERY_SHORT ? "short" : st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                fprintf(stderr, "s5pileup: read %.*s has no path: %s\n", (int)idl, id, why);
            }
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
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
    batch_close(&bt);
    slow5_close(in);
    free(st);
    free(acc); free(ref);
    return code;
}
