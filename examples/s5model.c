/*
 * s5model.c — a k-mer level table fitted to the reads of a file: the whole-read pileup of the file against the reference a FASTA file and
 * the current table make, folded onto k-mers on the GPU, and a new table estimated from the folded sums (k_pile_fold; docs/codecs.md §4.26).
 * What signal-level tools call a round of `train`.
 *
 *   s5model [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--tile T] [--band B] [--max-events N]
 *           [--refine [--refine-iters N] [--slope LO,HI]] [--iters N] [--min-cells M] [--fwd-only] --fasta ref.fa --model in.model -o out.model file.blow5
 *       <kmer>\t<level_mean>\t<level_stdv>\t<cells>\t<occurrences>\t<dwell>\t<kept>        one line per k-mer, in rank order, to out.model
 *   S, Q, M, T, B, N, --rna and the event parameters are those of s5extend; --refine, --refine-iters (s5extend's --iters) and --slope those
 *   of s5pileup --whole --refine: with them the sums are in the reference's units, which is what the estimate assumes.  in.model and --fwd-only
 *   are those of s5map --fasta.  A round makes the reference from the sequences and the current table, streams the file through the
 *   whole-read pileup handle, folds the table onto the 4^k k-mers when it closes it (s5gpu_pileup_close_folded) and solves
 *   (s5gpu_kmer_model_solve): level_mean = mu + (sd / scale) sum_q / cells, level_stdv = (sd / scale) sqrt(max(0, sumsq_q / cells - mean^2)),
 *   dwell = samples / cells; a k-mer with fewer than --min-cells cells (default 30) keeps its level and has kept = 1.  --iters N (1 .. 16,
 *   default 1) rounds, each from the table of the round before, which is out.model as it then stands.  occurrences: the reference columns
 *   that show the k-mer.  level_mean is the level rounded to float, printed as %.9g (a float survives it), level_stdv and dwell as %.6g.  In front stand a `#` line with
 *   k, the reads used in the last round and the rounds, and the column names; s5gpu_kmer_model_load reads the file back.
 *   Two limits: queries are clamped to +-127 (about +-4 sd), so a k-mer that far out is biased inwards; and the estimate is in the units
 *   of the table that made the reference, so a round changes the table's shape, not its overall scale.
 *   The totals of every round go to stderr.  Exit 0; 1 when a record is corrupt (its number goes to stderr; the other reads are counted);
 *   2 on any other error: a usage error, an unreadable model or FASTA, no segment.
 */
#define _GNU_SOURCE
#define S5TOOL "s5model"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not one of map's or extend's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
/* the batches of the file into the handle; 0, EXIT_CORRUPT or EXIT_ERROR */
static int add_file(void *h, const char *path, long K, int32_t *st) {
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    batch_t bt;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = s5gpu_pileup_add_batch_whole(h, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, NULL, NULL, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        for (uint32_t i = 0; i < n; i++)
            if (corrupt_status(st[i])) {
                fprintf(stderr, "s5model: record %" PRIu64 " of %s is corrupt (status %d)\n", bt.n_done + i, path, st[i]);
                code = EXIT_CORRUPT;
            }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    batch_close(&bt);
    slow5_close(in);
    return code;
}

int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, tile = 256, band = 512, emax = 1l << 20, r_iters = 2, rounds = 1, min_cells = 30;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, refine = 0, fwd_only = 0;
    const char *path = NULL, *fasta = NULL, *model = NULL, *out_path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--tile") && i + 1 < argc) tile = atol(argv[++i]);
        else if (!strcmp(argv[i], "--band") && i + 1 < argc) band = atol(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && i + 1 < argc) emax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--refine")) refine = 1;
        else if (!strcmp(argv[i], "--refine-iters") && i + 1 < argc) r_iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) rounds = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-cells") && i + 1 < argc) min_cells = atol(argv[++i]);
        else if (!strcmp(argv[i], "--fwd-only")) fwd_only = 1;
        else if (!strcmp(argv[i], "--fasta") && i + 1 < argc) fasta = argv[++i];
        else if (!strcmp(argv[i], "--model") && i + 1 < argc) model = argv[++i];
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) out_path = argv[++i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    const int tile_ok = tile == 64 || tile == 128 || tile == 256 || tile == 512 || tile == 1024;
    if (r_iters < 1 || r_iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) bad = 1;
    if (bad || !path || !fasta || !model || !out_path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 ||
        qmin > qmax || !tile_ok || band < 64 || band > 4096 || band % 64 != 0 || emax < qmin || emax > (1l << 20) || rounds < 1 || rounds > 16 || min_cells < 1 ||
        min_cells > 0xFFFFFFFFl) {
        fprintf(stderr, "usage: s5model [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--tile T (64, 128, 256, 512, 1024)]\n"
                        "               [--band B (a multiple of 64 in 64 .. 4096)] [--max-events N (M .. 2^20)]\n"
                        "               [--refine [--refine-iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)]] [--iters N (1 .. 16)] [--min-cells M (>= 1)]\n"
                        "               [--fwd-only] --fasta ref.fa --model in.model -o out.model file.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)r_iters};
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    if (!st) return die("out of memory");
    int code = EXIT_SUCCESS, gpu = 0;
    for (long round = 0; round < rounds; round++) {
        /* the current table: in.model, then out.model as the round before left it */
        const char *cur = round ? out_path : model;
        float *levels = NULL;
        uint32_t k = 0, R = 0, n4 = 0;
        if (s5gpu_kmer_model_load(cur, &levels, &k) != S5GPU_OK) return die("the model cannot be read");
        void *rs = s5gpu_refseq_open(fasta, cur, fwd_only ? 1 : 2, rna, M.scale, M.clip);
        if (!rs) return die("no reference from the sequences and the model");
        const int16_t *ref = s5gpu_refseq_ref(rs, &R);
        if (R > (1u << 26)) return die("the reference has more than 2^26 columns");
        double mu, sd, scale;
        uint32_t *cls = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)R);
        if (!cls) return die("out of memory");
        if (s5gpu_refseq_classes(rs, cls, &n4) != S5GPU_OK || s5gpu_refseq_quant(rs, &mu, &sd, &scale) != S5GPU_OK) return die("the reference has no classes");
        if (!gpu && s5gpu_init(0) != S5GPU_OK) return die("no GPU");
        gpu = 1;
        void *pile = s5gpu_pileup_open_whole(event_params(rna), &M, &B, 0, ref, R);
        if (!pile) return die("the table cannot be opened");
        if (refine && s5gpu_pileup_set_refine(pile, &RP) != S5GPU_OK) return die("the rounds cannot be turned on");
        const int c = add_file(pile, path, K, st);
        if (c == EXIT_ERROR) return EXIT_ERROR;
        if (c) code = c;
        uint8_t *acc = (uint8_t *)malloc(s5gpu_pileup_bytes(n4));
        s5gpu_kmer_row_t *rows = (s5gpu_kmer_row_t *)malloc(sizeof *rows * (size_t)n4);
        uint32_t *occ = (uint32_t *)calloc(n4, sizeof(uint32_t));
        if (!acc || !rows || !occ) return die("out of memory");
        if (s5gpu_pileup_close_folded(pile, cls, n4, acc) != S5GPU_OK) return die("the folded table cannot be fetched");
        const s5gpu_pile_total_t *T = (const s5gpu_pile_total_t *)acc;
        if (T->reserved[0] & S5GPU_FOLD_REFUSED) return die("the fold was refused: 2^32 cells or more");
        if (s5gpu_kmer_model_solve(acc, n4, mu, sd, scale, (uint32_t)min_cells, levels, rows) != S5GPU_OK) return die("the table cannot be solved");
        for (uint32_t j = 0; j < R; j++)
            if (cls[j] < n4) occ[cls[j]]++;
        FILE *o = fopen(out_path, "w");
        if (!o) { fprintf(stderr, "s5model: cannot write %s\n", out_path); return EXIT_ERROR; }
        fprintf(o, "# s5model k=%u reads_used=%" PRIu64 " rounds=%ld\nkmer\tlevel_mean\tlevel_stdv\tcells\toccurrences\tdwell\tkept\n", k, T->reads_used, round + 1);
        uint32_t n_kept = 0;
        for (uint32_t r = 0; r < n4; r++) {
            char kmer[16];
            for (uint32_t b = 0; b < k; b++) kmer[b] = "ACGT"[(r >> (2 * (k - 1 - b))) & 3u];
            kmer[k] = 0;
            fprintf(o, "%s\t%.9g\t%.6g\t%u\t%u\t%.6g\t%u\n", kmer, (double)(float)rows[r].level, rows[r].stdv, rows[r].cells, occ[r], rows[r].dwell, rows[r].kept);
            n_kept += rows[r].kept;
        }
        if (fclose(o) != 0) { fprintf(stderr, "s5model: write failed\n"); return EXIT_ERROR; }
        fprintf(stderr, "s5model: round %ld: reads used %" PRIu64 ", skipped %" PRIu64 ", bad %" PRIu64 "; cells %" PRIu64 ", cost %" PRIu64 "; %u columns, %u of %u k-mers kept\n",
                round + 1, T->reads_used, T->reads_skipped, T->reads_bad, T->cells, T->cost, R, n_kept, n4);
        free(acc); free(rows); free(occ); free(cls);
        s5gpu_refseq_close(rs);
        s5gpu_kmer_model_free(levels);
    }
    free(st);
    return code;
}
