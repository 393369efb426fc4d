/*
 * s5events.c — the events of every read of a BLOW5 file: scrappie-style segmentation (two sliding t-tests and a peak detector) made on the
 * GPU where the decoder left the read (k_sig_events, docs/codecs.md §4.15).
 *
 *   s5events [-K batch] [--rna] [--pa] file.blow5
 *       <read_id>\t<event>\t<start>\t<end>\t<mean>\t<stdv>       one line per event, reads in file order, events in order; `end` is
 *                                                                exclusive; mean and stdv as %.6g, raw units or (--pa) picoamperes
 *   Parameters: DNA 3, 6, 1.4, 9.0, 0.2; --rna 7, 14, 2.5, 9.0, 1.0.
 *   Exit 0; 1 when a record is corrupt (its read id, or its number in the file when the id cannot be read, goes to stderr; the other reads
 *   are printed); 2 on any other error (unreadable or damaged file, a .slow5 argument: text input is not built, convert it first).
 *
 * At most K records (default 4096) go to one s5gpu_signal_events_batch call: compressed bytes go up, 16 bytes per event come back.  The read
 * ids come from the device id path over the same records framed in one buffer; zstd records and ids longer than its pitch are the first
 * column of a skim line (batch_ids of s5tool.h).
 */
#define _GNU_SOURCE
#define S5TOOL "s5events"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2 };

static int corrupt_status(int32_t s) { return s != 0; }

int main(int argc, char **argv) {
    long K = 4096;
    int rna = 0, pa = 0, bad = 0;
    const char *path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--pa")) pa = 1;
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (bad || !path || K < 1 || K > (1l << 24)) {
        fprintf(stderr, "usage: s5events [-K batch] [--rna] [--pa] file.blow5\n");
        return EXIT_ERROR;
    }
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    const s5gpu_event_params_t *P = event_params(rna);
    const int mode = pa ? S5GPU_NORM_PA : S5GPU_NORM_RAW;
    big_stdout();

    batch_t bt;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    uint64_t *first = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)K + 1));
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    size_t rows_cap = 1 << 16;
    s5gpu_event_t *rows = (s5gpu_event_t *)malloc(sizeof(s5gpu_event_t) * rows_cap);
    if (!first || !st || !rows) return die("out of memory");
    int code = EXIT_SUCCESS;
    int64_t n;
    while ((n = batch_next(&bt)) > 0) {
        int rc = s5gpu_signal_events_batch((uint32_t)n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, mode, rows, rows_cap, first, st);
        if (rc == S5GPU_ERR_NOMEM) {
            rows_cap = (size_t)first[0] + (size_t)first[0] / 4;
            free(rows);
            rows = (s5gpu_event_t *)malloc(sizeof(s5gpu_event_t) * rows_cap);
            if (!rows) return die("out of memory");
            rc = s5gpu_signal_events_batch((uint32_t)n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, P, mode, rows, rows_cap, first, st);
        }
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("event detection failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < (uint32_t)n; i++) {
            if (st[i] != 0) { batch_corrupt(&bt, i, st[i]); code = EXIT_CORRUPT; continue; }
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            for (uint64_t e = first[i]; e < first[i + 1]; e++)
                printf("%.*s\t%" PRIu64 "\t%u\t%u\t%.6g\t%.6g\n", (int)idl, id, e - first[i], rows[e].start, rows[e].start + rows[e].length,
                       (double)rows[e].mean, (double)rows[e].stdv);
        }
        batch_release(&bt);
    }
    if (n < 0) return EXIT_ERROR;
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5events: write failed\n"); return EXIT_ERROR; }
    batch_close(&bt);
    slow5_close(in);
    free(first); free(st); free(rows);
    return code;
}
