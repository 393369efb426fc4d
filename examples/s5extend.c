/*
 * s5extend.c — where a WHOLE read lies on a reference squiggle: the first events of the read are mapped by subsequence DTW (s5map), and from
 * the column where they start the path of all its events is followed in tiles over a band of the reference that moves with it, on the GPU
 * (k_sdtw, k_ev_query_long, k_sdtw_band, k_sdtw_band_trace; docs/codecs.md §4.21).
 *
 *   s5extend [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--tile T] [--band B] [--max-events N] [--per-event]
 *            [--refine [--iters N] [--slope LO,HI]] ref.txt file.blow5
 *       <read_id>\t<events_used>\t<cost>\t<cost_per_event>\t<ref_start>\t<ref_end>\t<tiles>\t<anchor>      one line per read, in file order
 *   ref.txt, S, Q, M, the event parameters and the read ids are those of s5map: Q events behind the first S are mapped, and their start is
 *   the anchor.  The long query is the events behind the first S, at most N (default and most 2^20) and at least M; T (64, 128, 256, 512 or
 *   1024; default 256) rows make a tile, B (a multiple of 64 in 64 .. 4096; default 512) columns its window.  cost is the sum of
 *   |query - reference| over the path, cost_per_event = cost / events_used as %.3f; ref_start .. ref_end (inclusive) the reference positions
 *   of the first and the last event.  The band is a heuristic: a read whose true path leaves it is aligned worse, not refused, and
 *   cost_per_event is the only sign.  A read without a path prints `*` in every column behind its id, and why goes to stderr: `short`
 *   (fewer than M events), `row` (no anchor, or the walk failed), `wide` (the read's scratch alone is above 1 GiB).
 *   --per-event prints s5align's lines instead, for every event of the whole read:
 *       <read_id>\t<event>\t<sample_start>\t<sample_end>\t<mean>\t<ref_lo>\t<ref_hi>
 *   --refine (docs/codecs.md §4.24): behind the alignment, N rounds (1 .. 4; default 2) of: a per-read line reference = scale x query + shift
 *   fitted along the path (slopes in [LO, HI], default 0.5,2), the query requantised with it and aligned again in the band from ref_start.  The
 *   line gets the columns of s5refine behind it, formatted as there:
 *       ...\t<scale>\t<shift>\t<rounds>\t<cost_refined>\t<ref_start_refined>\t<ref_end_refined>\t<fit>
 *   fit is `ok`, or why the rounds ended early (`flat`, `range`, `row`): the columns then hold the last round that succeeded.  --per-event
 *   lines come from the refined path.
 *   Exit 0; 1 when a record is corrupt (its read id, or its number in the file when the id cannot be read, goes to stderr; the other reads
 *   are printed); 2 on any other error (an empty or unparsable reference, an unreadable or damaged file, a .slow5 argument: text input is
 *   not built, convert it first).
 *
 * At most K records (default 4096) go to one s5gpu_extend_batch call: compressed bytes go up; the rows, lo, hi and the event rows come
 * back in one download, ragged.  The read ids come from batch_ids of s5tool.h.
 */
#define _GNU_SOURCE
#define S5TOOL "s5extend"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's or align's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, tile = 256, band = 512, emax = 1l << 20, iters = 2;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, per_event = 0, refine = 0;
    const char *ref_path = NULL, *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--tile") && i + 1 < argc) tile = atol(argv[++i]);
        else if (!strcmp(argv[i], "--band") && i + 1 < argc) band = atol(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && i + 1 < argc) emax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--per-event")) per_event = 1;
        else if (!strcmp(argv[i], "--refine")) refine = 1;
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    const int tile_ok = tile == 64 || tile == 128 || tile == 256 || tile == 512 || tile == 1024;
    if (iters < 1 || iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) {
        fprintf(stderr, "s5extend: --iters N (1 .. 4), --slope LO,HI (0 < LO <= HI)\n");
        return EXIT_ERROR;
    }
    if (bad || !path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax || !tile_ok ||
        band < 64 || band > 4096 || band % 64 != 0 || emax < qmin || emax > (1l << 20)) {
        fprintf(stderr, "usage: s5extend [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--tile T (64, 128, 256, 512, 1024)]\n"
                        "                [--band B (a multiple of 64 in 64 .. 4096)] [--max-events N (M .. 2^20)] [--per-event]\n"
                        "                [--refine [--iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)]] ref.txt file.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)iters};
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
    s5gpu_map_row_t *map_rows = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K);
    s5gpu_ext_row_t *rows = (s5gpu_ext_row_t *)malloc(sizeof(s5gpu_ext_row_t) * (size_t)K);
    uint64_t *first = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
    s5gpu_ext_row_t *rows1 = (s5gpu_ext_row_t *)malloc(sizeof(s5gpu_ext_row_t) * (size_t)K);      /* --refine: the rows of the first alignment */
    s5gpu_fit_t *fit = (s5gpu_fit_t *)malloc(sizeof(s5gpu_fit_t) * (size_t)K);
    uint32_t *rounds = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)K);
    if (!st || !map_rows || !rows || !first || !rows1 || !fit || !rounds) return die("out of memory");
    size_t cap = 0;
    int32_t *lo = NULL, *hi = NULL;
    s5gpu_event_t *ev = NULL;
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        int rc = S5GPU_ERR_NOMEM;
        for (int attempt = 0; attempt < 2 && rc == S5GPU_ERR_NOMEM; attempt++) {                       /* the second time with the room the first asked for */
            if (refine)
                rc = s5gpu_extend_refine_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, &B, &RP, 0, ref, (uint32_t)R, map_rows, rows1, rows, first, lo, hi,
                                               per_event ? ev : NULL, NULL, cap, fit, rounds, st);
            else
                rc = s5gpu_extend_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, &B, 0, ref, (uint32_t)R, map_rows, rows, first, lo, hi,
                                        per_event ? ev : NULL, cap, st);
            if (rc != S5GPU_ERR_NOMEM || first[0] <= cap) break;
            cap = (size_t)first[0];
            free(lo); free(hi); free(ev);
            lo = (int32_t *)malloc(sizeof(int32_t) * cap); hi = (int32_t *)malloc(sizeof(int32_t) * cap);
            ev = per_event ? (s5gpu_event_t *)malloc(sizeof(s5gpu_event_t) * cap) : NULL;
            if (!lo || !hi || (per_event && !ev)) return die("out of memory");
        }
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < n; i++) {
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            if (corrupt_status(st[i])) {
                batch_corrupt(&bt, i, st[i]);
                code = EXIT_CORRUPT;
            } else if (refine ? rows1[i].status != 0 || rows1[i].qlen == 0 : st[i] != 0) {
                if (refine) st[i] = rows1[i].status ? rows1[i].status : S5GPU_STATUS_QUERY_SHORT;
                const char *why = st[i] == S5GPU_STATUS_QUERY_SHORT ? "short" : st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                fprintf(stderr, "s5extend: read %.*s has no path: %s\n", (int)idl, id, why);
                printf(per_event ? "%.*s\t*\t*\t*\t*\t*\t*\n" : refine ? "%.*s\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\t*\n" : "%.*s\t*\t*\t*\t*\t*\t*\t*\n",
                       (int)idl, id);
            } else if (per_event) {
                const size_t at = (size_t)first[i];
                for (uint32_t k = 0; k < rows[i].qlen; k++) {
                    const s5gpu_event_t *e = &ev[at + k];
                    printf("%.*s\t%" PRIu64 "\t%u\t%" PRIu64 "\t%.6g\t%d\t%d\n", (int)idl, id, (uint64_t)skip + k, e->start, (uint64_t)e->start + e->length,
                           (double)e->mean, lo[at + k], hi[at + k]);
                }
            } else if (refine) {
                const char *how = st[i] == 0 ? "ok" : st[i] == S5GPU_STATUS_FIT_FLAT ? "flat" : st[i] == S5GPU_STATUS_FIT_RANGE ? "range" : "row";
                printf("%.*s\t%u\t%" PRIu64 "\t%.3f\t%d\t%d\t%u\t%d\t%.9g\t%.9g\t%u\t%" PRIu64 "\t%d\t%d\t%s\n", (int)idl, id, rows1[i].qlen, rows1[i].cost,
                       (double)rows1[i].cost / (double)rows1[i].qlen, rows1[i].start, rows1[i].end, rows1[i].tiles, map_rows[i].start, fit[i].a, fit[i].b, rounds[i],
                       rows[i].cost, rows[i].start, rows[i].end, how);
            } else {
                printf("%.*s\t%u\t%" PRIu64 "\t%.3f\t%d\t%d\t%u\t%d\n", (int)idl, id, rows[i].qlen, rows[i].cost, (double)rows[i].cost / (double)rows[i].qlen,
                       rows[i].start, rows[i].end, rows[i].tiles, map_rows[i].start);
            }
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5extend: write failed\n"); return EXIT_ERROR; }
    batch_close(&bt);
    slow5_close(in);
    free(st);
    free(rows1); free(fit); free(rounds);
    free(map_rows); free(rows); free(first); free(lo); free(hi); free(ev); free(ref);
    return code;
}
