/*
 * s5contrast.c — where two samples differ: per reference position, the level histograms of the whole-read alignments of two files held
 * against each other on the GPU (k_pile_hist_accum, k_pile_contrast; docs/codecs.md §4.23).
 *
 *   s5contrast [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--tile T] [--band B] [--max-events N] [--min-depth D] [--q0 V] [--shift S]
 *              [--refine [--iters N] [--slope LO,HI]] ref.txt a.blow5 b.blow5
 *       <ref_pos>\t<ref_level>\t<depth_a>\t<depth_b>\t<events_a>\t<events_b>\t<mean_a>\t<mean_b>\t<ks_d>\t<ks_level>\t<tv>\t<med_a>\t<med_b>
 *   one line per position whose depth is at least D (default 1) in both files.  ref.txt, S, Q, M, T, B, N and the event parameters are those
 *   of s5extend.  depth, events and mean (sum / events, of the quantised event levels) come from each file's table as in s5pileup --whole.
 *   The histograms have 64 bins of 2^shift levels from q0 on (defaults -128 and 2: the clip of +-127 in bins of 4).  ks_d is the two-sample
 *   Kolmogorov-Smirnov statistic of the position's two histograms, ks_num / (events_a events_b), and tv their total-variation distance,
 *   1 - ov_num / (events_a events_b); ks_level is the lowest level of the bin where the two distributions are furthest apart, med_a and med_b
 *   the lowest level of each median's bin (q0 + (bin << shift)).  Doubles are printed as %.6g.  ks_d is a statistic, not a probability.
 *   The totals of both files (reads used, skipped, bad; cells; cost) go to stderr, a line each.
 *   --refine [--iters N] [--slope LO,HI]: every read of both files is first put into the reference's units by the rounds of
 *   s5extend --refine (docs/codecs.md §4.24; s5gpu_contrast_set_refine): a per-read scale error no longer shows as a level difference.  A
 *   read whose fit is refused is left out and counts as skipped; how many there were goes to stderr behind each file's totals.
 *   s5contrast ... --fasta ref.fa --model kmer.model [--fwd-only] [--by-kmer] a.blow5 b.blow5 : the reference is made from the sequences and
 *   the k-mer level table as in s5map --fasta (no ref.txt then); ref_pos is the reference column.  --by-kmer (docs/codecs.md §4.26): both
 *   files' tables and histograms are folded onto the 4^k k-mers on the GPU before they are compared (s5gpu_contrast_close_folded), one line
 *   per k-mer in rank order, the same thirteen columns: the k-mer stands where ref_pos stood and the table's quantised level for it where
 *   ref_level stood; depth and events are the sums over the columns that show the k-mer.  A shift that no single position has the depth
 *   to show can show here.
 *   Exit 0; 1 when a record is corrupt (its file and number go to stderr; the other reads are counted); 2 on any other error.
 *
 * One handle (s5gpu_contrast_open), one s5gpu_contrast_add_batch per K records (default 4096) of a.blow5, then of b.blow5, and one
 * s5gpu_contrast_close: compressed bytes go up; a status per read comes back, and the rows and the two tables once at the end.
 */
#define _GNU_SOURCE
#define S5TOOL "s5contrast"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's or extend's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
/* the batches of one file into `side` of the handle; 0, EXIT_CORRUPT or EXIT_ERROR */
static int add_file(void *h, int side, const char *path, long K, int32_t *st, uint64_t *n_refused) {
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    batch_t bt;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    bt.path_in_messages = 1;
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = s5gpu_contrast_add_batch(h, side, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, NULL, NULL, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        for (uint32_t i = 0; i < n; i++) {
            if (corrupt_status(st[i])) {
                fprintf(stderr, "s5contrast: record %" PRIu64 " of %s is corrupt (status %d)\n", bt.n_done + i, path, st[i]);
                code = EXIT_CORRUPT;
            }
            if (st[i] == S5GPU_STATUS_FIT_FLAT || st[i] == S5GPU_STATUS_FIT_RANGE) (*n_refused)++;
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    batch_close(&bt);
    slow5_close(in);
    return code;
}

int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, min_depth = 1, tile = 256, band = 512, emax = 1l << 20, q0 = -128, shift = 2;
    long iters = 2;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, refine = 0, fwd_only = 0, by_kmer = 0;
    const char *ref_path = NULL, *path[2] = {NULL, NULL}, *fasta = NULL, *model = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--min-depth") && i + 1 < argc) min_depth = atol(argv[++i]);
        else if (!strcmp(argv[i], "--tile") && i + 1 < argc) tile = atol(argv[++i]);
        else if (!strcmp(argv[i], "--band") && i + 1 < argc) band = atol(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && i + 1 < argc) emax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--q0") && i + 1 < argc) q0 = atol(argv[++i]);
        else if (!strcmp(argv[i], "--shift") && i + 1 < argc) shift = atol(argv[++i]);
        else if (!strcmp(argv[i], "--refine")) refine = 1;
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (!strcmp(argv[i], "--fasta") && i + 1 < argc) fasta = argv[++i];
        else if (!strcmp(argv[i], "--model") && i + 1 < argc) model = argv[++i];
        else if (!strcmp(argv[i], "--fwd-only")) fwd_only = 1;
        else if (!strcmp(argv[i], "--by-kmer")) by_kmer = 1;
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path[0]) path[0] = argv[i];
        else if (argv[i][0] != '-' && !path[1]) path[1] = argv[i];
        else bad = 1;
    }
    if (iters < 1 || iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) {
        fprintf(stderr, "s5contrast: --iters N (1 .. 4), --slope LO,HI (0 < LO <= HI)\n");
        return EXIT_ERROR;
    }
    if (fasta || model) {                                                  /* the reference is made here: the two positional arguments are the files */
        if (!fasta || !model || path[1]) bad = 1;
        path[1] = path[0]; path[0] = ref_path; ref_path = NULL;
    } else if (fwd_only || by_kmer) bad = 1;
    if (tile != 64 && tile != 128 && tile != 256 && tile != 512 && tile != 1024) bad = 1;
    if (band < 64 || band > 4096 || band % 64 || emax < qmin || emax > (1l << 20)) bad = 1;
    if (q0 < -32768 || q0 > 32767 || shift < 0 || shift > 10) bad = 1;
    if (bad || !path[1] || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax || min_depth < 1 ||
        min_depth > 0xFFFFFFFFl) {
        fprintf(stderr, "usage: s5contrast [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--tile T (64, 128, 256, 512, 1024)]\n"
                        "                  [--band B (a multiple of 64 in 64 .. 4096)] [--max-events N (M .. 2^20)] [--min-depth D (>= 1)]\n"
                        "                  [--q0 V (-32768 .. 32767)] [--shift S (0 .. 10)]\n"
                        "                  [--refine [--iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)]] ref.txt a.blow5 b.blow5\n"
                        "       s5contrast [...] --fasta ref.fa --model kmer.model [--fwd-only] [--by-kmer] a.blow5 b.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    size_t R = 0;
    int16_t *ref = NULL;
    void *rs = NULL;
    if (fasta) {
        rs = s5gpu_refseq_open(fasta, model, fwd_only ? 1 : 2, rna, M.scale, M.clip);
        if (!rs) return die("no reference from the sequences and the model");
        uint32_t R32 = 0;
        const int16_t *r = s5gpu_refseq_ref(rs, &R32);
        if (R32 > (1u << 22)) return die("the reference has more than 2^22 columns");
        R = R32;
        ref = (int16_t *)malloc(sizeof(int16_t) * R);
        if (!ref) return die("out of memory");
        memcpy(ref, r, sizeof(int16_t) * R);
    } else {
        float *levels = read_reference(ref_path, 1u << 22, "too many numbers (at most 2^22)", &R);
        if (!levels) return EXIT_ERROR;
        ref = (int16_t *)malloc(sizeof(int16_t) * R);
        if (!ref) return die("out of memory");
        if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
        free(levels);
    }
    /* --by-kmer: a class per column, and what is printed has a row per class */
    uint32_t n4 = 0, kk = 0, *cls = NULL;
    int16_t *kmer_q = NULL;
    if (by_kmer) {
        cls = (uint32_t *)malloc(sizeof(uint32_t) * R);
        if (!cls) return die("out of memory");
        if (s5gpu_refseq_classes(rs, cls, &n4) != S5GPU_OK || s5gpu_refseq_params(rs, &kk, NULL, NULL) != S5GPU_OK) return die("the reference has no classes");
        kmer_q = (int16_t *)calloc(n4, sizeof(int16_t));                     /* the quantised level of a k-mer: that of any column that shows it */
        if (!kmer_q) return die("out of memory");
        for (size_t j = 0; j < R; j++)
            if (cls[j] < n4) kmer_q[cls[j]] = ref[j];
    }
    const size_t N = by_kmer ? n4 : R;                                     /* the rows that come back */
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    big_stdout();

    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    uint8_t *acc[2] = {(uint8_t *)malloc(s5gpu_pileup_bytes((uint32_t)N)), (uint8_t *)malloc(s5gpu_pileup_bytes((uint32_t)N))};
    s5gpu_pile_contrast_t *rows = (s5gpu_pile_contrast_t *)malloc(sizeof *rows * N);
    if (!st || !acc[0] || !acc[1] || !rows) return die("out of memory");
    void *h = s5gpu_contrast_open(event_params(rna), &M, &B, 0, ref, (uint32_t)R, (int32_t)q0, (uint32_t)shift);
    if (!h) return die("the tables cannot be opened");
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)iters};
    if (refine && s5gpu_contrast_set_refine(h, &RP) != S5GPU_OK) return die("the rounds cannot be turned on");
    uint64_t n_refused[2] = {0, 0};
    int code = EXIT_SUCCESS;
    for (int side = 0; side < 2; side++) {
        const int c = add_file(h, side, path[side], K, st, &n_refused[side]);
        if (c == EXIT_ERROR) return EXIT_ERROR;
        if (c) code = c;
    }
    if ((by_kmer ? s5gpu_contrast_close_folded(h, cls, n4, acc[0], acc[1], rows) : s5gpu_contrast_close(h, acc[0], acc[1], rows)) != S5GPU_OK)
        return die("the rows cannot be fetched");
    const s5gpu_pile_col_t *ca = (const s5gpu_pile_col_t *)(acc[0] + sizeof(s5gpu_pile_total_t)), *cb = (const s5gpu_pile_col_t *)(acc[1] + sizeof(s5gpu_pile_total_t));
    for (size_t j = 0; j < N; j++) {
        const s5gpu_pile_contrast_t *r = &rows[j];
        if (r->depth_a < (uint64_t)min_depth || r->depth_b < (uint64_t)min_depth) continue;
        const double nn = (double)r->n_a * (double)r->n_b;
        if (by_kmer) {
            char kmer[16];
            for (uint32_t b = 0; b < kk; b++) kmer[b] = "ACGT"[(j >> (2 * (kk - 1 - b))) & 3u];
            kmer[kk] = 0;
            printf("%s\t%d\t%u\t%u\t%u\t%u\t%.6g\t%.6g\t%.6g\t%ld\t%.6g\t%ld\t%ld\n", kmer, (int)kmer_q[j], r->depth_a, r->depth_b, ca[j].n_events, cb[j].n_events,
                   (double)ca[j].sum_q / (double)ca[j].n_events, (double)cb[j].sum_q / (double)cb[j].n_events, (double)r->ks_num / nn, q0 + ((long)r->ks_bin << shift),
                   1.0 - (double)r->ov_num / nn, q0 + ((long)r->med_a << shift), q0 + ((long)r->med_b << shift));
            continue;
        }
        printf("%zu\t%d\t%u\t%u\t%u\t%u\t%.6g\t%.6g\t%.6g\t%ld\t%.6g\t%ld\t%ld\n", j, (int)ref[j], r->depth_a, r->depth_b, ca[j].n_events, cb[j].n_events,
               (double)ca[j].sum_q / (double)ca[j].n_events, (double)cb[j].sum_q / (double)cb[j].n_events, (double)r->ks_num / nn, q0 + ((long)r->ks_bin << shift),
               1.0 - (double)r->ov_num / nn, q0 + ((long)r->med_a << shift), q0 + ((long)r->med_b << shift));
    }
    for (int side = 0; side < 2; side++) {
        const s5gpu_pile_total_t *T = (const s5gpu_pile_total_t *)acc[side];
        fprintf(stderr, "s5contrast: %s: reads used %" PRIu64 ", skipped %" PRIu64 ", bad %" PRIu64 "; cells %" PRIu64 ", cost %" PRIu64 "; %zu positions\n", path[side],
                T->reads_used, T->reads_skipped, T->reads_bad, T->cells, T->cost, R);
        if (refine) fprintf(stderr, "s5contrast: %s: reads refused by the fit %" PRIu64 " (they count as skipped)\n", path[side], n_refused[side]);
    }
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5contrast: write failed\n"); return EXIT_ERROR; }
    free(st); free(acc[0]); free(acc[1]); free(rows); free(ref); free(cls); free(kmer_q);
    if (rs) s5gpu_refseq_close(rs);
    return code;
}
