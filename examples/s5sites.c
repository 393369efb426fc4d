/*
 * s5sites.c — which reads differ at a position: the level of every read at chosen reference positions, from its whole-read alignment, each
 * held against the level histogram of a control file at that position, on the GPU (k_site_cells, k_site_score; docs/codecs.md §4.25).
 *
 *   s5sites [-K batch] [--rna] [--skip S] [--events Q] [--min-events M] [--tile T] [--band B] [--max-events N] [--q0 V] [--shift S]
 *           [--refine [--iters N] [--slope LO,HI]] [--control ctl.blow5] --sites FILE ref.txt file.blow5
 *       <read_id>\t<ref_pos>\t<cells>\t<level>\t<first_event>\t<below>\t<above>\t<n>\t<tail>
 *   one line per read and position with cells > 0, reads in file order, positions ascending.  FILE holds one reference position per line
 *   (empty lines and lines that start with '#' skipped); the list is sorted and de-duplicated, at most 65536 positions, and a position at or
 *   beyond the end of ref.txt is refused.  ref.txt, S, Q, M, T, B, N and the event parameters are those of s5extend.  cells is the number of
 *   the read's events whose path crosses the position, level the mean of their quantised levels rounded half up, first_event the first of
 *   them, numbered as s5extend --per-event numbers events.
 *   --control: the control file is streamed first into a histogram of 64 bins of 2^shift levels from q0 on (defaults -128 and 2, as
 *   s5contrast).  With b the bin of level, below and above count the control's cells at the position in bins <= b and >= b, n all of them,
 *   and tail = min(1, 2 min(below, above) / n) as %.6g (`.` where n is 0).  tail is an empirical tail share, not a calibrated probability; a
 *   read that is itself in the control counts among its own control.  Without --control the last four columns are `.`.
 *   --refine [--iters N] [--slope LO,HI]: every read of both files is first put into the reference's units by the rounds of
 *   s5extend --refine (docs/codecs.md §4.24; s5gpu_sites_set_refine).  A read whose fit is refused is left out.
 *   The totals (the control's reads used, skipped, bad and cells; the file's reads, those with a line, and the lines) go to stderr.
 *   Exit 0; 1 when a record is corrupt (its file and number go to stderr; the other reads are counted); 2 on any other error.
 *
 * One handle (s5gpu_sites_open), one s5gpu_sites_add_control per K records (default 4096) of the control, one s5gpu_sites_add_batch per K
 * records of the file, whose cells and scores come back [positions][records], and one s5gpu_sites_close.
 */
#define _GNU_SOURCE
#define S5TOOL "s5sites"
#define S5TOOL_DIE 2
#include "s5tool.h"

enum { EXIT_CORRUPT = 1, EXIT_ERROR = 2, SITES_MOST = 65536 };

/* a status of the decoder's, not one of map's or extend's */
static int corrupt_status(int32_t s) {
    return s != 0 && s != S5GPU_STATUS_QUERY_SHORT && s != S5GPU_STATUS_PATH_WIDE && s != S5GPU_STATUS_PATH_ROW && s != S5GPU_STATUS_FIT_FLAT &&
           s != S5GPU_STATUS_FIT_RANGE;
}
static int by_column(const void *a, const void *b) {
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}
/* the site list: one column per line, sorted and de-duplicated; NULL (and a message) on a line that is no column, none, too many, one >= R */
static uint32_t *read_sites(const char *path, size_t R, uint32_t *m_out) {
    FILE *f = fopen(path, "r");
    if (!f) { fprintf(stderr, "s5sites: cannot open %s\n", path); return NULL; }
    size_t n = 0, cap = 1024, line_cap = 0, line_no = 0;
    uint32_t *v = (uint32_t *)malloc(sizeof(uint32_t) * cap);
    char *line = NULL;
    ssize_t l;
    while (v && (l = getline(&line, &line_cap, f)) >= 0) {
        line_no++;
        while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r' || line[l - 1] == ' ' || line[l - 1] == '\t')) line[--l] = 0;
        if (l == 0 || line[0] == '#') continue;
        char *end = NULL;
        const unsigned long long x = strtoull(line, &end, 10);
        if (end == line || *end != 0 || line[0] == '-' || line[0] == '+') {
            fprintf(stderr, "s5sites: %s line %zu is not a position\n", path, line_no);
            free(v); free(line); fclose(f);
            return NULL;
        }
        if (x >= R) {
            fprintf(stderr, "s5sites: %s line %zu: position %llu, the reference has %zu\n", path, line_no, x, R);
            free(v); free(line); fclose(f);
            return NULL;
        }
        if (n == cap) {
            cap *= 2;
            uint32_t *w = (uint32_t *)realloc(v, sizeof(uint32_t) * cap);
            if (!w) free(v);
            v = w;
        }
        if (v) v[n++] = (uint32_t)x;
    }
    free(line);
    fclose(f);
    if (!v) { fprintf(stderr, "s5sites: out of memory\n"); return NULL; }
    qsort(v, n, sizeof(uint32_t), by_column);
    size_t m = 0;
    for (size_t i = 0; i < n; i++)
        if (m == 0 || v[i] != v[m - 1]) v[m++] = v[i];
    if (m == 0 || m > SITES_MOST) { fprintf(stderr, "s5sites: %s holds %s\n", path, m ? "too many positions (at most 65536)" : "no position"); free(v); return NULL; }
    *m_out = (uint32_t)m;
    return v;
}

int main(int argc, char **argv) {
    long K = 4096, skip = 0, qmax = 250, qmin = 50, tile = 256, band = 512, emax = 1l << 20, q0 = -128, shift = 2, iters = 2;
    double a_lo = 0.5, a_hi = 2.0;
    int rna = 0, bad = 0, refine = 0;
    const char *ref_path = NULL, *path = NULL, *ctl_path = NULL, *sites_path = NULL;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-K") && i + 1 < argc) K = atol(argv[++i]);
        else if (!strcmp(argv[i], "--skip") && i + 1 < argc) skip = atol(argv[++i]);
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) qmax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--min-events") && i + 1 < argc) qmin = atol(argv[++i]);
        else if (!strcmp(argv[i], "--rna")) rna = 1;
        else if (!strcmp(argv[i], "--tile") && i + 1 < argc) tile = atol(argv[++i]);
        else if (!strcmp(argv[i], "--band") && i + 1 < argc) band = atol(argv[++i]);
        else if (!strcmp(argv[i], "--max-events") && i + 1 < argc) emax = atol(argv[++i]);
        else if (!strcmp(argv[i], "--q0") && i + 1 < argc) q0 = atol(argv[++i]);
        else if (!strcmp(argv[i], "--shift") && i + 1 < argc) shift = atol(argv[++i]);
        else if (!strcmp(argv[i], "--refine")) refine = 1;
        else if (!strcmp(argv[i], "--iters") && i + 1 < argc) iters = atol(argv[++i]);
        else if (!strcmp(argv[i], "--slope") && i + 1 < argc) { if (sscanf(argv[++i], "%lf,%lf", &a_lo, &a_hi) != 2) bad = 1; }
        else if (!strcmp(argv[i], "--control") && i + 1 < argc) ctl_path = argv[++i];
        else if (!strcmp(argv[i], "--sites") && i + 1 < argc) sites_path = argv[++i];
        else if (argv[i][0] != '-' && !ref_path) ref_path = argv[i];
        else if (argv[i][0] != '-' && !path) path = argv[i];
        else bad = 1;
    }
    if (iters < 1 || iters > 4 || !(a_lo > 0.0) || !(a_lo <= a_hi) || !(a_hi <= 1e300)) {
        fprintf(stderr, "s5sites: --iters N (1 .. 4), --slope LO,HI (0 < LO <= HI)\n");
        return EXIT_ERROR;
    }
    if (tile != 64 && tile != 128 && tile != 256 && tile != 512 && tile != 1024) bad = 1;
    if (band < 64 || band > 4096 || band % 64 || emax < qmin || emax > (1l << 20)) bad = 1;
    if (q0 < -32768 || q0 > 32767 || shift < 0 || shift > 10) bad = 1;
    if (bad || !path || !sites_path || K < 1 || K > (1l << 24) || skip < 0 || skip > 0x7FFFFFFFl || qmax < 1 || qmax > 1024 || qmin < 1 || qmin > qmax) {
        fprintf(stderr, "usage: s5sites [-K batch] [--rna] [--skip S] [--events Q (1 .. 1024)] [--min-events M (1 .. Q)] [--tile T (64, 128, 256, 512, 1024)]\n"
                        "               [--band B (a multiple of 64 in 64 .. 4096)] [--max-events N (M .. 2^20)] [--q0 V (-32768 .. 32767)] [--shift S (0 .. 10)]\n"
                        "               [--refine [--iters N (1 .. 4)] [--slope LO,HI (0 < LO <= HI)]] [--control ctl.blow5] --sites FILE ref.txt file.blow5\n");
        return EXIT_ERROR;
    }
    const s5gpu_map_params_t M = {(uint32_t)skip, (uint32_t)qmax, (uint32_t)qmin, 32.0, 127, 1};
    size_t R = 0;
    float *levels = read_reference(ref_path, 1u << 22, "too many numbers (at most 2^22)", &R);
    if (!levels) return EXIT_ERROR;
    uint32_t n_sites = 0;
    uint32_t *sites = read_sites(sites_path, R, &n_sites);
    if (!sites) return EXIT_ERROR;
    if ((uint64_t)n_sites * (uint64_t)K > (1ull << 27)) {                    /* the matrix of a batch: at most 2^27 entries */
        K = (long)((1ull << 27) / n_sites);
        fprintf(stderr, "s5sites: %u positions: batches of %ld records\n", n_sites, K);
    }
    int16_t *ref = (int16_t *)malloc(sizeof(int16_t) * R);
    if (!ref) return die("out of memory");
    if (s5gpu_quantise_host(levels, R, M.scale, M.clip, ref) != S5GPU_OK) return die("the reference cannot be quantised");
    free(levels);
    if (s5gpu_init(0) != S5GPU_OK) return die("no GPU");
    const s5gpu_band_params_t B = {(uint32_t)skip, (uint32_t)qmin, (uint32_t)emax, (uint32_t)tile, (uint32_t)band, M.clip, M.scale};
    big_stdout();

    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)K);
    s5gpu_site_cell_t *cells = (s5gpu_site_cell_t *)malloc(sizeof *cells * (size_t)K * n_sites);
    s5gpu_site_score_t *scores = (s5gpu_site_score_t *)malloc(sizeof *scores * (size_t)K * n_sites);
    if (!st || !cells || !scores) return die("out of memory");
    void *h = s5gpu_sites_open(event_params(rna), &M, &B, 0, ref, (uint32_t)R, sites, n_sites, (int32_t)q0, (uint32_t)shift);
    if (!h) return die("the handle cannot be opened");
    const s5gpu_refine_params_t RP = {a_lo, a_hi, 64.0, 127, 16, 16, (uint32_t)iters};
    if (refine && s5gpu_sites_set_refine(h, &RP) != S5GPU_OK) return die("the rounds cannot be turned on");
    int code = EXIT_SUCCESS;
    int64_t nb;
    batch_t bt;
    if (ctl_path) {
        slow5_file_t *ctl = open_blow5(ctl_path, NULL);
        if (!ctl) return EXIT_ERROR;
        if (batch_open(&bt, ctl, ctl_path, K) != 0) return EXIT_ERROR;
        bt.path_in_messages = 1;
        while ((nb = batch_next(&bt)) > 0) {
            const uint32_t n = (uint32_t)nb;
            const int rc = s5gpu_sites_add_control(h, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, st);
            if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment of the control failed");
            for (uint32_t i = 0; i < n; i++)
                if (corrupt_status(st[i])) {
                    fprintf(stderr, "s5sites: record %" PRIu64 " of %s is corrupt (status %d)\n", bt.n_done + i, ctl_path, st[i]);
                    code = EXIT_CORRUPT;
                }
            batch_release(&bt);
        }
        if (nb < 0) return EXIT_ERROR;
        batch_close(&bt);
        slow5_close(ctl);
    }
    slow5_file_t *in = open_blow5(path, NULL);
    if (!in) return EXIT_ERROR;
    if (batch_open(&bt, in, path, K) != 0) return EXIT_ERROR;
    bt.path_in_messages = 1;
    uint64_t n_reads = 0, n_with = 0, n_lines = 0;
    while ((nb = batch_next(&bt)) > 0) {
        const uint32_t n = (uint32_t)nb;
        const int rc = s5gpu_sites_add_batch(h, n, (const void *const *)bt.mem, bt.len, bt.rec, bt.sig, NULL, cells, scores, st);
        if (rc != S5GPU_OK && rc != S5GPU_ERR_DATA) return die("alignment failed");
        if (batch_ids(&bt, st, corrupt_status, 0) != 0) return EXIT_ERROR;
        for (uint32_t i = 0; i < n; i++) {
            n_reads++;
            if (corrupt_status(st[i])) {
                fprintf(stderr, "s5sites: record %" PRIu64 " of %s is corrupt (status %d)\n", bt.n_done + i, path, st[i]);
                code = EXIT_CORRUPT;
                continue;
            }
            size_t idl;
            const char *id = batch_id(&bt, i, &idl);
            int any = 0;
            for (uint32_t t = 0; t < n_sites; t++) {
                const s5gpu_site_cell_t *c = &cells[(size_t)t * n + i];
                if (c->cells == 0) continue;
                any = 1;
                n_lines++;
                const s5gpu_site_score_t *s = &scores[(size_t)t * n + i];     /* (against an empty control without --control: the level alone) */
                printf("%.*s\t%u\t%u\t%d\t%" PRIu64, (int)idl, id, sites[t], c->cells, (int)s->level, (uint64_t)skip + c->row0);
                if (!ctl_path) { printf("\t.\t.\t.\t.\n"); continue; }
                const uint32_t least = s->below < s->above ? s->below : s->above;
                const double tail = s->n ? 2.0 * (double)least / (double)s->n : 0.0;
                if (s->n) printf("\t%u\t%u\t%u\t%.6g\n", s->below, s->above, s->n, tail < 1.0 ? tail : 1.0);
                else printf("\t%u\t%u\t%u\t.\n", s->below, s->above, s->n);
            }
            n_with += (uint64_t)any;
        }
        batch_release(&bt);
    }
    if (nb < 0) return EXIT_ERROR;
    batch_close(&bt);
    slow5_close(in);
    s5gpu_pile_hist_head_t *hist = (s5gpu_pile_hist_head_t *)malloc(s5gpu_pile_hist_bytes((uint32_t)R));
    if (!hist) return die("out of memory");
    if (s5gpu_sites_close(h, hist) != S5GPU_OK) return die("the control cannot be fetched");
    if (ctl_path)
        fprintf(stderr, "s5sites: %s: reads used %" PRIu64 ", skipped %" PRIu64 ", bad %" PRIu64 "; cells %" PRIu64 "; %zu positions\n", ctl_path, hist->reads_used,
                hist->reads_skipped, hist->reads_bad, hist->cells, R);
    fprintf(stderr, "s5sites: %s: reads %" PRIu64 ", with a line %" PRIu64 "; lines %" PRIu64 "; %u sites\n", path, n_reads, n_with, n_lines, n_sites);
    if (fflush(stdout) != 0 || ferror(stdout)) { fprintf(stderr, "s5sites: write failed\n"); return EXIT_ERROR; }
    free(hist); free(st); free(cells); free(scores); free(sites); free(ref);
    return code;
}
