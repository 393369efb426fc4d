/*
 * s5stats.c — what `slow5tools stats` prints of a SLOW5 / BLOW5 file, and, with --signal, what is in the file's signal: the file-wide
 * accumulator of docs/codecs.md §4.13, made on the GPU while the records stream through it.
 *
 *   s5stats file.[b|s]low5
 *       the reference's nine lines (src/stats.c): file path (as given), version, format, the two presses, read groups, auxiliary fields
 *       (count and names; a file without any prints a bare "auxiliary fields" line) and the number of records.  No GPU call is made: the
 *       records of a BLOW5 file are counted by their framing (reader_t of s5tool.h, here over plain memory), those of a SLOW5 file
 *       line by line (textbatch_t, the same way).  Exit 1 with a message on a file that cannot be opened, whose version is above 1.0.0,
 *       with a damaged frame or without the end-of-file marker.
 *   s5stats --signal [--hist FILE] [-K batch] file.[b|s]low5
 *       the nine lines, then tab-separated lines from the accumulator:
 *         total samples, sample min, sample max, sample sum, sample sum of squares (modulo 2^64), constant low bits (the trailing zero bits
 *         all samples share: 16 when every sample is 0), sample median / 1st percentile / 99th percentile (the value at rank
 *         floor(q (N - 1)) of the sorted samples, from the histogram), sample mean (%.3f), read length min, read length max,
 *         `reads of length class b <tab> count` for every class in use (class 0: no samples, else 1 + floor(log2 n)),
 *         `read group g <tab> reads <tab> samples` for every read group of the header (below 256).
 *       A value that does not exist (no samples, no reads) prints as ".".  --hist FILE: `value <tab> count` for every value that occurs, in
 *       value order.  At most K records (default 4096) go to one s5gpu_file_stats_add_stream call; nothing comes back until the end.
 *       A SLOW5 ASCII file has its lines converted to BLOW5 records with both presses none by s5gpu_ascii_to_blow5_stream first, as in s5sum.
 *       A record that does not decode: exit 1, and nothing of the signal section is printed.
 */
#define _GNU_SOURCE
#define S5TOOL "s5stats"
#include "s5tool.h"

static int fail(const char *what) {
    fprintf(stderr, "s5stats: %s\n", what);
    return -1;
}
static int fail_gpu(const char *what) {
    complain(what);
    return -1;
}

static int report_bad_record(const int32_t *status, uint32_t n) {
    for (uint32_t i = 0; i < n; i++)
        if (status[i]) { fprintf(stderr, "s5stats: record %u of a batch is corrupt (status %d)\n", i, status[i]); break; }
    return -1;
}

/* the records of a BLOW5 file: counted, and with h added to its accumulator */
static int walk_blow5(slow5_file_t *in, const char *path, uint32_t K, size_t chunk, void *h, int64_t *count) {
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    reader_t R;
    int32_t *st = NULL;
    int rc = -1;
    if (reader_open(&R, in, path, K, chunk, h != NULL) != 0) { fail("cannot read the records (no end-of-file marker, or out of memory)"); goto done; }
    if (h && !(st = (int32_t *)malloc(sizeof(int32_t) * K))) { fail("out of memory"); goto done; }
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) { fail("damaged record framing"); goto done; }
        if (n == 0) break;
        *count += n;
        if (!h) continue;
        const int arc = s5gpu_file_stats_add_stream(h, (uint32_t)n, R.buf, R.have, R.rec_pos, R.rec_len, rec, sig, st);
        if (arc == S5GPU_ERR_DATA) { report_bad_record(st, (uint32_t)n); goto done; }
        if (arc != S5GPU_OK) { fail_gpu("the statistics call failed"); goto done; }
    }
    rc = 0;
done:
    reader_close(&R);
    free(st);
    return rc;
}

/* the record lines of a SLOW5 ASCII file: counted; with h, K lines at a time -> BLOW5 records (none, none) on the device -> back -> the accumulator */
static int walk_slow5(slow5_file_t *in, uint32_t K, size_t chunk, void *h, int64_t *count) {
    const struct slow5_aux_meta *am = in->header->aux_meta;
    textbatch_t T;
    size_t ocap = chunk;
    uint8_t *out = NULL;
    uint64_t *off = NULL, *rec_pos = NULL;
    uint32_t *rec_len = NULL;
    int32_t *st = NULL;
    int rc = -1;
    if (textbatch_open(&T, K, chunk, h != NULL) != 0) goto done;
    out = h ? (uint8_t *)s5gpu_host_alloc(ocap) : NULL;
    off = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
    rec_pos = (uint64_t *)malloc(sizeof(uint64_t) * K);
    rec_len = (uint32_t *)malloc(sizeof(uint32_t) * K);
    st = (int32_t *)malloc(sizeof(int32_t) * K);
    if ((h && !out) || !off || !rec_pos || !rec_len || !st) { fail_gpu("out of memory"); goto done; }
    for (;;) {
        const int64_t nl = textbatch_next(&T, in);
        if (nl < 0) goto done;
        if (nl == 0) break;
        const uint32_t n = (uint32_t)nl;
        *count += n;
        if (!h) continue;
        int arc = s5gpu_ascii_to_blow5_stream(n, T.txt, T.have, T.line_pos, T.line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                              NULL, 0, out, ocap, off, st);
        if (arc == S5GPU_ERR_NOMEM) {
            const size_t need = (size_t)off[0];
            s5gpu_host_free(out);
            ocap = need + need / 4;
            out = (uint8_t *)s5gpu_host_alloc(ocap);
            if (!out) { fail_gpu("out of memory"); goto done; }
            arc = s5gpu_ascii_to_blow5_stream(n, T.txt, T.have, T.line_pos, T.line_len, am ? am->num : 0, am ? am->types : NULL, S5GPU_REC_NONE, S5GPU_SIG_NONE,
                                              NULL, 0, out, ocap, off, st);
        }
        if (arc != S5GPU_OK) { fail_gpu("a record line cannot be parsed"); goto done; }
        for (uint32_t i = 0; i < n; i++) { rec_pos[i] = off[i] + 8; rec_len[i] = (uint32_t)(off[i + 1] - off[i] - 8); }
        arc = s5gpu_file_stats_add_stream(h, n, out, (size_t)off[n], rec_pos, rec_len, S5GPU_REC_NONE, S5GPU_SIG_NONE, st);
        if (arc == S5GPU_ERR_DATA) { report_bad_record(st, n); goto done; }
        if (arc != S5GPU_OK) { fail_gpu("the statistics call failed"); goto done; }
    }
    rc = 0;
done:
    textbatch_close(&T);
    if (out) s5gpu_host_free(out);
    free(off); free(rec_pos); free(rec_len); free(st);
    return rc;
}

/* the names of the auxiliary fields: the columns behind raw_signal of the header's column line */
static void print_aux_fields(const slow5_hdr_t *hd) {
    const char *h = hd->data, *names = NULL;
    size_t len = hd->data_len, names_len = 0, b = 0;
    while (b < len) {
        const char *e = (const char *)memchr(h + b, '\n', len - b);
        const size_t l = e ? (size_t)(e - h) - b : len - b;
        if (l >= 9 && memcmp(h + b, "#read_id\t", 9) == 0) {
            static const char key[] = "\traw_signal\t";
            const char *at = (const char *)memmem(h + b, l, key, sizeof key - 1);
            if (at) { names = at + sizeof key - 1; names_len = l - (size_t)(names - (h + b)); }
        }
        b += l + 1;
    }
    if (!hd->aux_meta || !names || names_len == 0) {       /* the reference's exception: no tab and no names behind the label */
        printf("number of auxiliary fields\t%d\nauxiliary fields\n", 0);
        return;
    }
    uint32_t num = 1;
    for (size_t i = 0; i < names_len; i++) num += names[i] == '\t';
    printf("number of auxiliary fields\t%u\nauxiliary fields\t", num);
    for (size_t i = 0; i < names_len; i++) putchar(names[i] == '\t' ? ',' : names[i]);
    putchar('\n');
}

/* the value at rank floor(q (N - 1)) of the sorted samples */
static int hist_quantile(const s5gpu_file_stats_t *A, double q) {
    const double t = q * (double)(A->n_samples - 1);
    uint64_t rank = t > 0.0 ? (uint64_t)t : 0, seen = 0;
    if (rank > A->n_samples - 1) rank = A->n_samples - 1;
    for (int b = 0; b < 65536; b++) {
        seen += A->hist[b];
        if (rank < seen) return b - 32768;
    }
    return 32767;
}

static void print_signal(const s5gpu_file_stats_t *A, uint32_t n_groups) {
    const int any = A->n_samples != 0;
    printf("total samples\t%" PRIu64 "\n", A->n_samples);
    if (any) printf("sample min\t%d\nsample max\t%d\n", A->min, A->max);
    else printf("sample min\t.\nsample max\t.\n");
    printf("sample sum\t%" PRId64 "\nsample sum of squares\t%" PRIu64 "\n", A->sum, A->sumsq);
    printf("constant low bits\t%d\n", A->or_bits ? __builtin_ctz(A->or_bits) : 16);
    if (any) {
        printf("sample median\t%d\nsample 1st percentile\t%d\nsample 99th percentile\t%d\n", hist_quantile(A, 0.5), hist_quantile(A, 0.01), hist_quantile(A, 0.99));
        printf("sample mean\t%.3f\n", (double)A->sum / (double)A->n_samples);
    } else printf("sample median\t.\nsample 1st percentile\t.\nsample 99th percentile\t.\nsample mean\t.\n");
    if (A->n_reads) printf("read length min\t%u\nread length max\t%u\n", A->len_min, A->len_max);
    else printf("read length min\t.\nread length max\t.\n");
    for (int b = 0; b < 33; b++)
        if (A->len_hist[b]) printf("reads of length class %d\t%" PRIu64 "\n", b, A->len_hist[b]);
    for (uint32_t g = 0; g < n_groups && g < 256; g++) printf("read group %u\t%" PRIu64 "\t%" PRIu64 "\n", g, A->rg_reads[g], A->rg_samples[g]);
    if (A->rg_other) printf("read groups 256 and above\t%" PRIu64 "\n", A->rg_other);
}

int main(int argc, char **argv) {
    int want_signal = 0, bad = 0;
    long K = 4096;
    const char *path = NULL, *hist_path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--signal")) want_signal = 1;
        else if (!strcmp(argv[i], "--hist") && i + 1 < argc) hist_path = argv[++i];
        else if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (bad || !path || K < 1 || K > (1l << 24) || (hist_path && !want_signal)) {
        fprintf(stderr, "usage: s5stats file.[b|s]low5\n       s5stats --signal [--hist FILE] [-K batch] file.[b|s]low5\n");
        return EXIT_FAILURE;
    }
    printf("file path\t%s\n", path);
    int ret = EXIT_FAILURE;
    void *h = NULL;
    s5gpu_file_stats_t *A = NULL;
    slow5_file_t *in = slow5_open(path, "r");              /* tells BLOW5 from SLOW5 ASCII by the file's first bytes */
    if (!in) { fflush(stdout); fprintf(stderr, "s5stats: cannot open %s\n", path); return EXIT_FAILURE; }
    const struct slow5_version v = in->header->version;
    if (v.major > 1 || (v.major == 1 && (v.minor > 0 || v.patch > 0))) {
        fflush(stdout);
        fprintf(stderr, "s5stats: file version %d.%d.%d is above 1.0.0, the last this tool reads\n", v.major, v.minor, v.patch);
        goto done;
    }
    const enum slow5_press_method rm = in->compress->record_press->method, sm = in->compress->signal_press->method;
    const uint32_t n_groups = in->header->num_read_groups;
    printf("file version\t%d.%d.%d\n", v.major, v.minor, v.patch);
    printf("file format\t%s\n", in->format == SLOW5_FORMAT_ASCII ? "SLOW5 ASCII" : in->format == SLOW5_FORMAT_BINARY ? "BLOW5" : "FORMAT_UNKNOWN");
    printf("record compression method\t%s\n", rm == SLOW5_COMPRESS_NONE ? "none" : rm == SLOW5_COMPRESS_ZLIB ? "zlib" : rm == SLOW5_COMPRESS_ZSTD ? "zstd" : "compression error");
    printf("signal compression method\t%s\n", sm == SLOW5_COMPRESS_NONE ? "none" : sm == SLOW5_COMPRESS_SVB_ZD ? "svb-zd" : sm == SLOW5_COMPRESS_EX_ZD ? "ex-zd" : "compression error");
    printf("number of read groups\t%u\n", n_groups);
    print_aux_fields(in->header);
    fflush(stdout);

    if (want_signal) {
        if (s5gpu_init(0) != S5GPU_OK) { fail_gpu("no GPU"); goto done; }
        if (!(h = s5gpu_file_stats_open())) { fail_gpu("cannot make the accumulator"); goto done; }
    }
    const size_t chunk = (size_t)64 << 20;
    int64_t count = 0;
    if ((in->format == SLOW5_FORMAT_BINARY ? walk_blow5(in, path, (uint32_t)K, chunk, h, &count) : walk_slow5(in, (uint32_t)K, chunk, h, &count)) != 0) goto done;
    printf("number of records\t%" PRId64 "\n", count);
    if (want_signal) {
        if (!(A = (s5gpu_file_stats_t *)malloc(sizeof *A))) { fail("out of memory"); goto done; }
        const int crc = s5gpu_file_stats_close(h, A);      /* the handle ends here whatever this returns */
        h = NULL;
        if (crc != S5GPU_OK) { fail_gpu("cannot fetch the accumulator"); goto done; }
        if (A->n_failed) { fail("a record did not decode"); goto done; }
        print_signal(A, n_groups);
        if (hist_path) {
            FILE *hf = fopen(hist_path, "w");
            if (!hf) { fail("cannot write the histogram file"); goto done; }
            for (int b = 0; b < 65536; b++)
                if (A->hist[b]) fprintf(hf, "%d\t%" PRIu64 "\n", b - 32768, A->hist[b]);
            if (fclose(hf) != 0) { fail("cannot write the histogram file"); goto done; }
        }
    }
    if (fflush(stdout) != 0 || ferror(stdout)) { fail("write failed"); goto done; }
    ret = EXIT_SUCCESS;
done:
    if (h) (void)s5gpu_file_stats_close(h, NULL);
    free(A);
    slow5_close(in);
    return ret;
}
