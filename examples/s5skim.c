/*
 * s5skim.c — `slow5tools skim` (src/skim.c) on the GPU press path: every field of every read but the raw signal.
 *
 *   s5skim [--rid | --hdr] [-K batch] in.blow5
 *       (default)  a column line, then one line per record in file order (src/skim.c:340-420).  The file is read in chunks straight
 *                  into pinned memory and framed in place; at most K records (default 4096, src/cmd.h) go to one s5gpu_skim_stream call,
 *                  which inflates them on the device, formats the lines there and returns them as one block of text.
 *       --rid      the read ids, one per line, in file order (src/skim.c:31-51).  Ids come from the device id path
 *                  (idsrc_t of s5tool.h; zstd records and ids longer than its pitch take the default mode's path); no .idx file is
 *                  written.  A repeated id is an error, as slow5_idx_load makes it in the reference.
 *       --hdr      the header as SLOW5 ASCII (src/skim.c:54-57).
 *   Output goes to stdout.  SLOW5 ASCII input is refused.  S5SKIM_CHUNK_KB (tests): the chunk size.
 */
#define _GNU_SOURCE
#define S5TOOL "s5skim"
#define S5TOOL_DIE EXIT_FAILURE
#include "s5tool.h"

/* a batch that cannot be skimmed: which record, where the call says so */
static int skim_failed(int rc, const int32_t *status, uint32_t n) {
    if (rc == S5GPU_ERR_DATA) {
        for (uint32_t i = 0; i < n; i++)
            if (status[i]) { fprintf(stderr, "s5skim: record %u of the batch cannot be skimmed (status %d)\n", i, status[i]); break; }
    }
    return die("skim failed");
}

int main(int argc, char **argv) {
    int rid = 0, hdr = 0;
    long K = 4096;
    const char *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--rid")) rid = 1;
        else if (!strcmp(argv[i], "--hdr")) hdr = 1;
        else if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else { path = NULL; break; }
    }
    if (!path || K < 1 || K > (1l << 24)) {
        fprintf(stderr, "usage: s5skim [--rid | --hdr] [-K batch] in.blow5\n");
        return EXIT_FAILURE;
    }
    if (rid && hdr) { fprintf(stderr, "s5skim: --rid and --hdr cannot be used together\n"); return EXIT_FAILURE; }
    slow5_file_t *in = open_blow5(path, "is SLOW5 ASCII; s5skim reads BLOW5 files only");
    if (!in) return EXIT_FAILURE;
    if (hdr) {
        const slow5_press_method_t none = {SLOW5_COMPRESS_NONE, SLOW5_COMPRESS_NONE};
        if (slow5_hdr_fwrite(stdout, in->header, SLOW5_FORMAT_ASCII, none) < 0 || fflush(stdout) != 0) return die("cannot write the header");
        slow5_close(in);
        return EXIT_SUCCESS;
    }
    const int rec = rec_code_of(in->compress->record_press->method), sig = sig_code_of(in->compress->signal_press->method);
    s5gpu_skim_layout_t *L = (s5gpu_skim_layout_t *)calloc(1, sizeof *L);
    if (!L) return die("out of memory");
    if (rid ? rid_layout(in->header->data, in->header->data_len, L) != 0
            : s5gpu_skim_layout_parse(in->header->data, in->header->data_len, L) != S5GPU_OK)
        return die("the header cannot be skimmed");
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    size_t chunk = (size_t)64 << 20;
    const char *e = getenv("S5SKIM_CHUNK_KB");
    if (e && atoi(e) > 0) chunk = (size_t)atoi(e) << 10;
    reader_t R;
    if (reader_open(&R, in, path, (uint32_t)K, chunk, 1) != 0) return die("cannot read the records (no end-of-file marker, or out of memory)");

    if (rid) {                                             /* the ids in file order, a repeated one is an error */
        idsrc_t I;
        idlist_t ids;
        memset(&ids, 0, sizeof ids);
        if (idsrc_open(&I, in, (uint32_t)K) != 0) return EXIT_FAILURE;
        I.L = L;
        for (;;) {
            const int64_t n = next_batch(&R);
            if (n < 0) return die("damaged record framing");
            if (n == 0) break;
            const int rc = idsrc_batch(&I, &R, (uint32_t)n);
            if (rc == -1) return EXIT_FAILURE;
            if (rc != S5GPU_OK) return skim_failed(rc, I.txt.status, (uint32_t)n);
            for (uint32_t i = 0; i < (uint32_t)n; i++) {
                size_t l;
                const char *id = id_of(&I, i, &l);
                if (!id || idlist_add(&ids, id, l) != 0) return die("out of memory");
            }
        }
        const int64_t dup = idlist_index(&ids, NULL, NULL);
        if (dup == -2) return die("out of memory");
        if (dup >= 0) { complain_duplicate(&ids, dup, path); return EXIT_FAILURE; }
        for (uint64_t i = 0; i < ids.n; i++)
            if (puts(idlist_id(&ids, i)) < 0) return die("write failed");
        if (fflush(stdout) != 0) return die("write failed");
        return EXIT_SUCCESS;
    }

    lines_t o;
    o.cap = (size_t)K * 256 + 4096;
    o.p = (uint8_t *)s5gpu_host_alloc(o.cap);
    o.off = (uint64_t *)malloc(sizeof(uint64_t) * (K + 1));
    o.status = (int32_t *)malloc(sizeof(int32_t) * K);
    if (!o.p || !o.off || !o.status) return die("out of memory");
    /* default: the column line, a warning per field skim does not handle (src/skim.c:257), then the records */
    for (uint32_t a = 0; a < L->n_aux; a++)
        if (L->role[a] == S5GPU_SKIM_DOT)
            fprintf(stderr, "[WARNING] s5skim: Field '%.*s' is not yet handled or not present in the input file. A '.' will be printed\n",
                    (int)L->name_len[a], L->text + L->name_off[a]);
    fputs("#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal", stdout);
    for (uint32_t a = 0; a < L->n_aux; a++) printf("\t%.*s", (int)L->name_len[a], L->text + L->name_off[a]);
    fputc('\n', stdout);
    for (;;) {
        const int64_t n = next_batch(&R);
        if (n < 0) return die("damaged record framing");
        if (n == 0) break;
        const int rc = skim_lines(&R, (uint32_t)n, rec, sig, L, &o);
        if (rc != S5GPU_OK) return skim_failed(rc, o.status, (uint32_t)n);
        if (o.off[n] && fwrite(o.p, 1, o.off[n], stdout) != o.off[n]) return die("write failed");
    }
    if (fflush(stdout) != 0) return die("write failed");
    return EXIT_SUCCESS;
}
