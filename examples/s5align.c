/*
 * s5align.c — which reference positions each event of a read landed on: the whole path of the read's subsequence DTW alignment against a
 * reference squiggle, walked back on the GPU (k_sdtw, k_sdtw_dirs, k_sdtw_trace; docs/codecs.md §4.17).
 *
 *   s5align [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--max-span W] ref.txt file.blow5
 *       <read_id>\t<event>\t<sample_start>\t<sample_end>\t<mean>\t<ref_lo>\t<ref_hi>      one line per query event, reads in file order
 *   ref.txt, S, Q, M, the event parameters and the read ids are those of s5map.  event = S + i for row i of the query; sample_end is
 *   exclusive; mean is the event's mean of the raw signal as %.6g; ref_lo .. ref_hi (inclusive) are the reference positions the event is
 *   aligned to.  A read without a path prints one line with `*` in every column behind its id, and why goes to stderr: `short` (fewer
 *   than M events), `wide` (the alignment spans more than W reference positions; default 4 Q, at most 2^20: W bounds the scratch a read
 *   needs, not the quality).
 *   Exit 0; 1 when a record is corrupt (its read id, or its number in the file when the id cannot be read, goes to stderr; the other reads
 *   are printed); 2 on any other error (an empty or unparsable reference, an unreadable or damaged file, a .slow5 argument: text input is
 *   not built, convert it first).
 *
 * At most K records (default 4096) go to one s5gpu_align_batch call: compressed bytes go up; the rows, lo, hi and the query's event rows
 * come back in one download.  The read ids come from batch_ids of s5tool.h.
 */
#define _GNU_SOURCE
#define S5TOOL "s5align"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's or align's */
static int corrupt_status(int32_t s) { return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW; }
int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, wmax = -1;
    int rna = 0, bad = 0;
    const char *ref_path = NULL, *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--max-span") && i + 1 < argc) wmax = atol(argv[++i]);
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (wmax == -1) wmax = 4 * qmax;
    if (bad || !path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax || wmax < 1 ||
        wmax > (1l << 20)) {
        fprintf(stderr, "usage: s5align [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--max-span W (1 .. 2^20)] ref.txt file.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
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
    s5gpu_map_row_t *rows = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K);
    int32_t *lo = (int32_t *)malloc(sizeof(int32_t) * (size_t)K * (size_t)qmax), *hi = (int32_t *)malloc(sizeof(int32_t) * (size_t)K * (size_t)qmax);
    s5gpu_event_t *ev = (s5gpu_event_t *)malloc(sizeof(s5gpu_event_t) * (size_t)K * (size_t)qmax);
    if (!rows || !lo || !hi || !ev) return die("out of memory");
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = s5gpu_align_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, (uint32_t)wmax, ref, (uint32_t)R, rows, lo, hi, ev, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < n; i++) {
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            if (corrupt_status(st[i])) {
                batch_corrupt(&bt, i, st[i]);
                code = EXIT_CORRUPT;
            } else if (st[i] != 0) {
                const char *why = st[i] == S5GPU_STATUS_QUERY_SHORT ? "short" : st[i] == S5GPU_STATUS_PATH_WIDE ? "wide" : "row";
                fprintf(stderr, "s5align: read %.*s has no path: %s\n", (int)idl, id, why);
                printf("%.*s\t*\t*\t*\t*\t*\t*\n", (int)idl, id);
            } else {
                const size_t at = (size_t)i * (size_t)qmax;
                for (uint32_t k = 0; k < rows[i].qlen; k++) {
                    const s5gpu_event_t *e = &ev[at + k];
                    printf("%.*s\t%" PRIu64 "\t%u\t%" PRIu64 "\t%.6g\t%d\t%d\n", (int)idl, id, (uint64_t)skip + k, e->start, (uint64_t)e->start + e->length,
                           (double)e->mean, lo[at + k], hi[at + k]);
                }
            }
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5align: write failed\n"); return EXIT_ERROR; }
    batch_close(&bt);
    slow5_close(in);
    free(st);
    free(rows); free(lo); free(hi); free(ev); free(ref);
    return code;
}
