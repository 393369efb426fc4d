/*
 * s5map.c — where in a target each read of a BLOW5 file came from: subsequence DTW of the read's events against a reference squiggle, on the
 * GPU where the decoder left the read (k_sig_events, k_ev_query, k_sdtw; docs/codecs.md §4.16).
 *
 *   s5map [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--start] ref.txt file.blow5
 *       <read_id>\t<events_used>\t<cost>\t<cost_per_event>\t<ref_start>\t<ref_end>      one line per read, in file order
 *   ref.txt: the expected current levels of the target, made elsewhere (no pore model ships with this project): one number per line in
 *   strtod syntax, empty lines and lines that start with '#' skipped; read as float32 and quantised on the host (s5gpu_quantise_host).
 *   The first S (default 0) events of a read are left out, the next Q (default 250, at most 1024) are its query; a read with fewer than M
 *   (default 50, at most Q) prints `*` in every column behind its id.  cost_per_event = cost / events_used as %.6g; ref_end is inclusive;
 *   ref_start is `*` without --start.  Event parameters: DNA 3, 6, 1.4, 9.0, 0.2; --rna 7, 14, 2.5, 9.0, 1.0.
 *   Exit 0; 1 when a record is corrupt (its read id, or its number in the file when the id cannot be read, goes to stderr; the other reads
 *   are printed); 2 on any other error (an empty or unparsable reference, an unreadable or damaged file, a .slow5 argument: text input is
 *   not built, convert it first).
 *
 *   s5map ... --second [--block-shift b] ref.txt file.blow5
 *       the same line with \t<cost2>\t<ref_end2>\t<mapq> behind it: the best hit at least two blocks of 2^b columns away from the first
 *       (docs/codecs.md §4.19; b in 6 .. 30, default the smallest whose block holds Q columns) and mapq = 60 (cost2 - cost) / cost2, a
 *       separation ratio in 0 .. 60, no probability.  No such hit: `*`, `*` and 0; no query: `*` in all three.
 *   s5map ... --fasta ref.fa --model kmer.model [--fwd-only] [--block-shift b] file.blow5
 *       <read_id>\t<events_used>\t<cost>\t<cost_per_event>\t<contig>\t<strand>\t<pos_start>\t<pos_end>\t<mapq>\t<cost2>
 *       The reference is made from the sequences and the k-mer level table (s5gpu_refseq_open: one line per k-mer, `kmer level_mean`, all 4^k
 *       of them): per contig the forward levels, then those of the reverse complement (--fwd-only: not these; --rna: the forward levels
 *       reversed, nothing else).  Implies --start --second.  pos_start <= pos_end are 0-based k-mer starts on the forward strand.  Exit 2 for
 *       an unreadable or incomplete model, a FASTA without a sequence, or no contig of k bases.
 *
 * At most K records (default 4096) go to one s5gpu_map_batch call: compressed bytes go up, 16 bytes per read come back.  The read ids come
 * from the device id path over the same records framed in one buffer; zstd records and ids longer than its pitch are the first column of a
 * skim line (batch_ids of s5tool.h).
 */
#define _GNU_SOURCE
#define S5TOOL "s5map"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

/* a status of the decoder's, not map's */
static int corrupt_status(int32_t s) { return s != 0 && s != S5GPU_STATUS_QUERY_SHORT; }

/* the line of --fasta: the hit's columns as contig, strand and the first and last k-mer start on the forward strand (a span that is not
 * inside one segment, which the walls rule out, would print `*` there) */
static void print_located(const void *rs, const char *id, size_t idl, const s5gpu_map_row_t *r, const s5gpu_map_second_t *r2) {
    if (r->qlen == 0) { printf("%.*s\t*\t*\t*\t*\t*\t*\t*\t*\t*\n", (int)idl, id); return; }
    printf("%.*s\t%u\t%u\t%.6g\t", (int)idl, id, r->qlen, r->cost, (double)r->cost / (double)r->qlen);
    s5gpu_refseq_loc_t a, b;
    s5gpu_refseq_segment_t seg;
    if (r->start >= 0 && r->end >= 0 && s5gpu_refseq_locate(rs, (uint32_t)r->start, &a) == S5GPU_OK &&
        s5gpu_refseq_locate(rs, (uint32_t)r->end, &b) == S5GPU_OK && a.segment == b.segment && s5gpu_refseq_segment(rs, a.segment, &seg) == S5GPU_OK)
        printf("%s\t%c\t%u\t%u", seg.name, (char)a.strand, a.pos < b.pos ? a.pos : b.pos, a.pos < b.pos ? b.pos : a.pos);
    else printf("*\t*\t*\t*");
    if (r2->end2 >= 0) printf("\t%u\t%u\n", r2->mapq, r2->cost2);
    else printf("\t%u\t*\n", r2->mapq);
}

int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, bshift = 0;
    int rna = 0, want_start = 0, bad = 0, second = 0, fwd_only = 0;
    const char *ref_path = NULL, *path = NULL, *fasta = NULL, *model = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--second")) second = 1;
        else if (!strcmp(argv[i], "--block-shift") && i + 1 < argc) { bshift = atol(argv[++i]); if (bshift < 6 || bshift > 30) bad = 1; }
        else if (!strcmp(argv[i], "--fasta") && i + 1 < argc) fasta = argv[++i];
        else if (!strcmp(argv[i], "--model") && i + 1 < argc) model = argv[++i];
        else if (!strcmp(argv[i], "--fwd-only")) fwd_only = 1;
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--start")) want_start = 1;
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (fasta || model) {                                                  /* the reference is made here: the one positional argument is the file */
        if (!fasta || !model || path) bad = 1;
        path = ref_path; ref_path = NULL;
        want_start = second = 1;
    } else if (fwd_only) bad = 1;
    if (bshift && !second) bad = 1;
    if (bad || !path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax) {
        fprintf(stderr, "usage: s5map [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--start]\n"
                        "             [--second [--block-shift b (6 .. 30)]] ref.txt file.blow5\n"
                        "       s5map [...] --fasta ref.fa --model kmer.model [--fwd-only] [--block-shift b] file.blow5\n");
        return EXIT_ERROR;
    }
    if (!bshift)
        for (bshift = 6; (1l << bshift) < qmax; bshift++) {}               /* the smallest block that holds the query */
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, want_start};
    size_t R = 0;
    int16_t *ref = NULL;
    void *rs = NULL;
    if (fasta) {
        rs = s5gpu_refseq_open(fasta, model, fwd_only ? 1 : 2, rna, M.scale, M.clip);
        if (!rs) return die("no reference from the sequences and the model");
        uint32_t R32 = 0;
        ref = (int16_t *)s5gpu_refseq_ref(rs, &R32);
        R = R32;
    } else {
        float *levels = read_reference(ref_path, 0x7FFFFFFFu, "too many numbers", &R);
        if (!levels) return EXIT_ERROR;
        ref = (int16_t *)malloc(sizeof(int16_t) * R);
        if (!ref) return die("out of memory");
        if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
        free(levels);
    }
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    const s5gpu_event_params_t *P = event_params(rna);
    big_stdout();

    batch_t bt;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    s5gpu_map_row_t *rows = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K);
    s5gpu_map_second_t *rows2 = (s5gpu_map_second_t *)malloc(sizeof(s5gpu_map_second_t) * (size_t)K);
    if (!st || !rows || !rows2) return die("out of memory");
    int code = EXIT_SUCCESS;
    int64_t nb;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = second ? s5gpu_map2_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, ref, (uint32_t)R, (uint32_t)bshift, rows, rows2, st)
                              : s5gpu_map_batch(n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, &M, ref, (uint32_t)R, rows, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("mapping failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < n; i++) {
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            if (corrupt_status(st[i])) {
                batch_corrupt(&bt, i, st[i]);
                code = EXIT_CORRUPT;
            } else if (rs) {
                print_located(rs, id, idl, &rows[i], &rows2[i]);
            } else if (rows[i].qlen == 0) {
                printf("%.*s\t*\t*\t*\t*\t*%s\n", (int)idl, id, second ? "\t*\t*\t*" : "");
            } else {
                printf("%.*s\t%u\t%u\t%.6g\t", (int)idl, id, rows[i].qlen, rows[i].cost, (double)rows[i].cost / (double)rows[i].qlen);
                if (want_start) printf("%d\t%d", rows[i].start, rows[i].end);
                else printf("*\t%d", rows[i].end);
                if (second && rows2[i].end2 >= 0) printf("\t%u\t%d\t%u", rows2[i].cost2, rows2[i].end2, rows2[i].mapq);
                else if (second) printf("\t*\t*\t%u", rows2[i].mapq);
                putchar('\n');
            }
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5map: write failed\n"); return EXIT_ERROR; }
    batch_close(&bt);
    slow5_close(in);
    free(st); free(rows); free(rows2);
    if (rs) s5gpu_refseq_close(rs);
    else free(ref);
    return code;
}
