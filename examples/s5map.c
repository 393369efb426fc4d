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
 * from the device id path (s5gpu_record_ids_stream) over the same records framed in one buffer; zstd records and ids longer than its pitch
 * are the first column of a skim line (s5gpu_skim_batch).
 */
#define _GNU_SOURCE
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slow5_compat.h"
#include "slow5gpu.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2, PITCH = 128 };

static int die(const char *what) {
    fprintf(stderr, "s5map: %s (%s)\n", what, s5gpu_last_error());
    return EXIT_ERROR;
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
    if (!f) { fprintf(stderr, "s5map: cannot open %s\n", path); return NULL; }
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
            fprintf(stderr, "s5map: %s line %zu is not a number\n", path, line_no);
            free(v); free(line); fclose(f);
            return NULL;
        }
        if (n == cap) { cap *= 2; v = (float *)realloc(v, sizeof(float) * cap); }
        if (v) v[n++] = (float)x;
    }
    free(line);
    fclose(f);
    if (!v) { fprintf(stderr, "s5map: out of memory\n"); return NULL; }
    if (n == 0 || n > 0x7FFFFFFFu) { fprintf(stderr, "s5map: %s holds %s\n", path, n ? "too many numbers" : "no number"); free(v); return NULL; }
    *n_out = n;
    return v;
}

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
        float *levels = read_reference(ref_path, &R);
        if (!levels) return EXIT_ERROR;
        ref = (int16_t *)malloc(sizeof(int16_t) * R);
        if (!ref) return die("out of memory");
        if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
        free(levels);
    }
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    slow5_file_t *in = slow5_open(path, "r");
    if (!in) { fprintf(stderr, "s5map: cannot open %s\n", path); return EXIT_ERROR; }
    if (in->format != SLOW5_FORMAT_BINARY) { fprintf(stderr, "s5map: %s is SLOW5 text: convert it to BLOW5 first\n", path); return EXIT_ERROR; }
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
    s5gpu_map_row_t *rows = (s5gpu_map_row_t *)malloc(sizeof(s5gpu_map_row_t) * (size_t)K);
    uint8_t *chunk = NULL;
    s5gpu_skim_layout_t *L = NULL;
    s5gpu_map_second_t *rows2 = (s5gpu_map_second_t *)malloc(sizeof(s5gpu_map_second_t) * (size_t)K);
    if (!rows || !rows2) return die("out of memory");
    int code = EXIT_SUCCESS, at_end = 0;
    uint64_t n_done = 0;
    while (!at_end) {
        uint32_t n = 0;
        size_t bytes = 0;
        while (n < (uint32_t)K) {
            mem[n] = slow5_get_next_mem(&len[n], in);
            if (!mem[n]) {
                if (slow5_errno != SLOW5_ERR_EOF) { fprintf(stderr, "s5map: cannot read record %" PRIu64 " of %s\n", n_done + n, path); return EXIT_ERROR; }
                at_end = 1;
                break;
            }
            if (len[n] > 0xFFFFFF00u) { fprintf(stderr, "s5map: record %" PRIu64 " is too large\n", n_done + n); return EXIT_ERROR; }
            bytes += 8 + len[n];
            n++;
        }
        if (n == 0) break;
        const int rc = second ? s5gpu_map2_batch(n, (const void *const *)mem, len, rec, sig, P, &M, ref, (uint32_t)R, (uint32_t)bshift, rows, rows2, st)
                              : s5gpu_map_batch(n, (const void *const *)mem, len, rec, sig, P, &M, ref, (uint32_t)R, rows, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("mapping failed");
        /* the ids: the device id path over the records framed in one buffer; what it leaves (zstd, long ids) is the first column of a skim line */
        for (uint32_t i = 0; i < n; i++) ist[i] = 5;
        if (rec != S5GPU_REC_ZSTD) {
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
            if (ist[i] == 0 || (st[i] != 0 && st[i] != S5GPU_STATUS_QUERY_SHORT)) continue;              /* (a corrupt record has no skim line either) */
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
            if (st[i] != 0 && st[i] != S5GPU_STATUS_QUERY_SHORT) {
                if (id) fprintf(stderr, "s5map: read %.*s is corrupt (status %d)\n", (int)idl, id, st[i]);
                else fprintf(stderr, "s5map: record %" PRIu64 " of the file is corrupt (status %d)\n", n_done + i, st[i]);
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
            free(line[i]);
            free(mem[i]);
            mem[i] = NULL;
        }
        n_done += n;
    }
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5map: write failed\n"); return EXIT_ERROR; }
    if (chunk) s5gpu_host_free(chunk);
    slow5_close(in);
    free(mem); free(len); free(rec_pos); free(rec_len); free(st); free(ist); free(ids); free(id_len); free(line); free(line_len);
    free(rows); free(rows2); free(L);
    if (rs) s5gpu_refseq_close(rs);
    else free(ref);
    return code;
}
