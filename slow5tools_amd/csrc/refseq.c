/* refseq.c — a reference squiggle from sequences and a k-mer model, on the host (include/slow5gpu.h "a reference squiggle from sequences";
 * docs/codecs.md §4.19): the model file, the FASTA file, the levels of a contig, the segments in their order, the quantiser over all of
 * them together, the walls between them, and the way back from a column to contig, strand and position.  Plain C; no device is touched. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slow5gpu.h"

void s5gpu_set_error(const char *fmt, ...);

enum { KMAX = 10, WMAX = 64 };

typedef struct refseq {
    int16_t *ref;
    uint32_t R, k, W, n_contigs, n_seg;
    int32_t clip;
    char **names;
    uint64_t *len;
    uint32_t *Lk;
    s5gpu_refseq_segment_t *seg;
    uint32_t *cls;                                                         /* [R]: the rank of each column's k-mer, or S5GPU_FOLD_NONE (§4.26) */
    double mu, sd, scale;                                                  /* the quantiser's: over all segments' levels together */
} refseq_t;

/* A, C, G, T (U) = 0 .. 3 without case; anything else -1 */
static int base_code(char c) {
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return -1;
    }
}

/* ---------------------------------------------------------------------------------------------------------------- the model file */
int s5gpu_kmer_model_load(const char *path, float **levels_out, uint32_t *k_out) {
    const char *who = "s5gpu_kmer_model_load";
    if (!path || !levels_out || !k_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    *levels_out = NULL; *k_out = 0;
    FILE *f = fopen(path, "r");
    if (!f) { s5gpu_set_error("%s: cannot open %s", who, path); return S5GPU_ERR_ARG; }
    char *line = NULL;
    size_t cap = 0, line_no = 0, n4 = 0, seen_n = 0;
    ssize_t l;
    uint32_t k = 0;
    float *lev = NULL;
    uint8_t *seen = NULL;
    int rc = S5GPU_OK;
    while (rc == S5GPU_OK && (l = getline(&line, &cap, f)) >= 0) {
        line_no++;
        while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r' || line[l - 1] == ' ' || line[l - 1] == '\t')) line[--l] = 0;
        if (l == 0 || line[0] == '#' || strncmp(line, "kmer", 4) == 0) continue;
        size_t kl = 0, rank = 0;
        static const char acgt[] = "ACGT";                                 /* (a model's k-mers are upper case ACGT, nothing else) */
        const char *at;
        while (kl <= KMAX && line[kl] && (at = strchr(acgt, line[kl]))) {
            rank = rank * 4 + (size_t)(at - acgt);
            kl++;
        }
        if (kl == 0 || kl > KMAX || (line[kl] != ' ' && line[kl] != '\t')) {
            s5gpu_set_error("%s: %s line %zu does not start with a k-mer over ACGT of 1 .. %d bases and a level", who, path, line_no, KMAX);
            rc = S5GPU_ERR_DATA;
            break;
        }
        if (k == 0) {
            k = (uint32_t)kl;
            n4 = (size_t)1 << (2 * k);
            lev = (float *)malloc(sizeof(float) * n4);
            seen = (uint8_t *)calloc(n4, 1);
            if (!lev || !seen) { s5gpu_set_error("%s: out of memory", who); rc = S5GPU_ERR_NOMEM; break; }
        }
        if (kl != k) { s5gpu_set_error("%s: %s line %zu has a k-mer of %zu bases, the ones before it of %u", who, path, line_no, kl, k); rc = S5GPU_ERR_DATA; break; }
        char *end = NULL;
        const double x = strtod(line + kl, &end);
        if (end == line + kl || (*end != 0 && *end != ' ' && *end != '\t')) {
            s5gpu_set_error("%s: %s line %zu has no level behind its k-mer", who, path, line_no);
            rc = S5GPU_ERR_DATA;
            break;
        }
        if (seen[rank]) { s5gpu_set_error("%s: %s line %zu names a k-mer a second time", who, path, line_no); rc = S5GPU_ERR_DATA; break; }
        seen[rank] = 1; seen_n++;
        lev[rank] = (float)x;
    }
    free(line);
    fclose(f);
    if (rc == S5GPU_OK && (k == 0 || seen_n != n4)) {
        s5gpu_set_error("%s: %s holds %zu of the %zu k-mers of %u bases", who, path, seen_n, n4, k);
        rc = S5GPU_ERR_DATA;
    }
    free(seen);
    if (rc != S5GPU_OK) { free(lev); return rc; }
    *levels_out = lev; *k_out = k;
    return S5GPU_OK;
}

void s5gpu_kmer_model_free(float *levels) { free(levels); }

/* ---------------------------------------------------------------------------------------------------------------- levels */
/* the Lk = L - k + 1 levels of codes[0 .. L) (L >= k): the model's, or `mean` for a k-mer that holds a code of -1 */
static void levels_of(const int8_t *codes, size_t L, const float *model, uint32_t k, float mean, float *out) {
    const size_t maskk = ((size_t)1 << (2 * k)) - 1;
    size_t rank = 0;
    long long last_bad = -1;
    for (size_t p = 0; p < L; p++) {
        if (codes[p] < 0) last_bad = (long long)p;
        rank = ((rank << 2) | (size_t)(codes[p] < 0 ? 0 : codes[p])) & maskk;
        if (p + 1 >= k) {
            const size_t s = p + 1 - k;
            out[s] = last_bad >= (long long)s ? mean : model[rank];
        }
    }
}

/* ... and their ranks: the rank levels_of took the level of, S5GPU_FOLD_NONE where it took the mean */
static void classes_of(const int8_t *codes, size_t L, uint32_t k, uint32_t *out) {
    const size_t maskk = ((size_t)1 << (2 * k)) - 1;
    size_t rank = 0;
    long long last_bad = -1;
    for (size_t p = 0; p < L; p++) {
        if (codes[p] < 0) last_bad = (long long)p;
        rank = ((rank << 2) | (size_t)(codes[p] < 0 ? 0 : codes[p])) & maskk;
        if (p + 1 >= k) {
            const size_t s = p + 1 - k;
            out[s] = last_bad >= (long long)s ? S5GPU_FOLD_NONE : (uint32_t)rank;
        }
    }
}

static void refseq_free(refseq_t *h) {
    if (!h) return;
    if (h->names)
        for (uint32_t i = 0; i < h->n_contigs; i++) free(h->names[i]);
    free(h->names); free(h->len); free(h->Lk); free(h->seg); free(h->ref); free(h->cls); free(h);
}

void *s5gpu_refseq_build(uint32_t n_contigs, const char *const *names, const char *const *seqs, const size_t *lens, const float *model, uint32_t k,
                         int strands, int rna, double scale, int32_t clip) {
    const char *who = "s5gpu_refseq_build";
    if (!names || !seqs || !lens || !model || n_contigs == 0) { s5gpu_set_error("%s: NULL argument or no contig", who); return NULL; }
    if (k < 1 || k > KMAX) { s5gpu_set_error("%s: k = %u (1 .. %d)", who, k, KMAX); return NULL; }
    if (!rna && strands != 1 && strands != 2) { s5gpu_set_error("%s: strands = %d (1 or 2)", who, strands); return NULL; }
    int16_t probe = 0;
    const float one = 0.0f;
    if (s5gpu_quantise_host(&one, 1, scale, clip, &probe) != S5GPU_OK) return NULL;          /* (scale and clip: its message) */
    const uint32_t W = (2048u * (uint32_t)clip) / (32768u - (uint32_t)clip) + 1u;
    if (W > WMAX) { s5gpu_set_error("%s: a clip of %d needs walls of %u columns (at most %d)", who, clip, W, WMAX); return NULL; }
    const int per = rna ? 1 : strands;
    refseq_t *h = (refseq_t *)calloc(1, sizeof *h);
    if (!h) { s5gpu_set_error("%s: out of memory", who); return NULL; }
    h->k = k; h->W = W; h->clip = clip; h->n_contigs = n_contigs;
    h->names = (char **)calloc(n_contigs, sizeof(char *));
    h->len = (uint64_t *)calloc(n_contigs, sizeof(uint64_t));
    h->Lk = (uint32_t *)calloc(n_contigs, sizeof(uint32_t));
    h->seg = (s5gpu_refseq_segment_t *)calloc((size_t)n_contigs * (size_t)per, sizeof(s5gpu_refseq_segment_t));
    float *lev = NULL;
    int8_t *codes = NULL;
    int16_t *q = NULL;
    uint32_t *cls = NULL;
    if (!h->names || !h->len || !h->Lk || !h->seg) goto nomem;
    uint64_t total = 0, longest = 0;
    for (uint32_t i = 0; i < n_contigs; i++) {
        if (!names[i] || (!seqs[i] && lens[i])) { s5gpu_set_error("%s: contig %u is NULL", who, i); goto fail; }
        if (!(h->names[i] = strdup(names[i]))) goto nomem;
        h->len[i] = lens[i];
        if (lens[i] < k) continue;
        const uint64_t Lk = (uint64_t)lens[i] - k + 1;
        total += Lk * (uint64_t)per;
        if (total + (uint64_t)W * (uint64_t)n_contigs * 2u > 0x7FFFFFFFull) { s5gpu_set_error("%s: more than 2^31 - 1 columns", who); goto fail; }
        h->Lk[i] = (uint32_t)Lk;
        if (lens[i] > longest) longest = lens[i];
    }
    if (total == 0) { s5gpu_set_error("%s: no contig has %u bases: no segment", who, k); goto fail; }
    /* the table's mean: the double sum in rank order, divided, rounded to float */
    const size_t n4 = (size_t)1 << (2 * k);
    double sum = 0.0;
    for (size_t r = 0; r < n4; r++) sum += (double)model[r];
    const float mean = (float)(sum / (double)n4);
    lev = (float *)malloc(sizeof(float) * total);
    codes = (int8_t *)malloc(longest);
    q = (int16_t *)malloc(sizeof(int16_t) * total);
    cls = (uint32_t *)malloc(sizeof(uint32_t) * total);
    if (!lev || !codes || !q || !cls) goto nomem;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_contigs; i++) {
        const uint32_t Lk = h->Lk[i];
        const size_t L = lens[i];
        if (!Lk) continue;
        for (size_t p = 0; p < L; p++) codes[p] = (int8_t)base_code(seqs[i][p]);
        levels_of(codes, L, model, k, mean, lev + at);
        classes_of(codes, L, k, cls + at);
        if (rna)
            for (uint32_t a = 0, b = Lk - 1; a < b; a++, b--) {
                const float t = lev[at + a]; lev[at + a] = lev[at + b]; lev[at + b] = t;
                const uint32_t u = cls[at + a]; cls[at + a] = cls[at + b]; cls[at + b] = u;
            }
        s5gpu_refseq_segment_t *s = &h->seg[h->n_seg++];
        s->contig = i; s->strand = '+'; s->Lk = Lk; s->reversed = rna ? 1 : 0; s->name = h->names[i];
        at += Lk;
        if (per == 2) {
            for (size_t p = 0; p < L; p++) { const int c = base_code(seqs[i][L - 1 - p]); codes[p] = (int8_t)(c < 0 ? -1 : 3 - c); }
            levels_of(codes, L, model, k, mean, lev + at);
            classes_of(codes, L, k, cls + at);
            s = &h->seg[h->n_seg++];
            s->contig = i; s->strand = '-'; s->Lk = Lk; s->reversed = 1; s->name = h->names[i];
            at += Lk;
        }
    }
    if (s5gpu_quantise_host(lev, (size_t)total, scale, clip, q) != S5GPU_OK) goto fail;
    if (s5gpu_quant_stats_host(lev, (size_t)total, &h->mu, &h->sd) != S5GPU_OK) goto fail;
    h->scale = scale;
    h->R = (uint32_t)(total + (uint64_t)W * (h->n_seg - 1));
    h->ref = (int16_t *)malloc(sizeof(int16_t) * h->R);
    h->cls = (uint32_t *)malloc(sizeof(uint32_t) * h->R);
    if (!h->ref || !h->cls) goto nomem;
    uint32_t col = 0;
    at = 0;
    for (uint32_t s = 0; s < h->n_seg; s++) {
        if (s)
            for (uint32_t w = 0; w < W; w++) { h->cls[col] = S5GPU_FOLD_NONE; h->ref[col++] = INT16_MIN; }
        h->seg[s].offset = col;
        memcpy(h->ref + col, q + at, sizeof(int16_t) * h->seg[s].Lk);
        memcpy(h->cls + col, cls + at, sizeof(uint32_t) * h->seg[s].Lk);
        col += h->seg[s].Lk; at += h->seg[s].Lk;
    }
    free(lev); free(codes); free(q); free(cls);
    return h;
nomem:
    s5gpu_set_error("%s: out of memory", who);
fail:
    free(lev); free(codes); free(q); free(cls);
    refseq_free(h);
    return NULL;
}

/* ---------------------------------------------------------------------------------------------------------------- the FASTA file */
void *s5gpu_refseq_open(const char *fasta_path, const char *model_path, int strands, int rna, double scale, int32_t clip) {
    const char *who = "s5gpu_refseq_open";
    if (!fasta_path || !model_path) { s5gpu_set_error("%s: NULL argument", who); return NULL; }
    float *model = NULL;
    uint32_t k = 0;
    if (s5gpu_kmer_model_load(model_path, &model, &k) != S5GPU_OK) return NULL;
    FILE *f = fopen(fasta_path, "r");
    if (!f) { s5gpu_set_error("%s: cannot open %s", who, fasta_path); free(model); return NULL; }
    char **names = NULL, **seqs = NULL, *line = NULL;
    size_t *lens = NULL, *caps = NULL, n = 0, n_cap = 0, cap = 0;
    ssize_t l;
    void *h = NULL;
    int ok = 1;
    while (ok && (l = getline(&line, &cap, f)) >= 0) {
        if (l > 0 && line[0] == '>') {
            if (n == n_cap) {
                n_cap = n_cap ? n_cap * 2 : 16;
                names = (char **)realloc(names, sizeof(char *) * n_cap);
                seqs = (char **)realloc(seqs, sizeof(char *) * n_cap);
                lens = (size_t *)realloc(lens, sizeof(size_t) * n_cap);
                caps = (size_t *)realloc(caps, sizeof(size_t) * n_cap);
                if (!names || !seqs || !lens || !caps) { s5gpu_set_error("%s: out of memory", who); ok = 0; n = 0; break; }
            }
            size_t e = 1;
            while (e < (size_t)l && line[e] != ' ' && line[e] != '\t' && line[e] != '\n' && line[e] != '\r') e++;
            names[n] = strndup(line + 1, e - 1);
            seqs[n] = NULL; lens[n] = 0; caps[n] = 0;
            if (!names[n]) { s5gpu_set_error("%s: out of memory", who); ok = 0; break; }
            n++;
            continue;
        }
        for (ssize_t p = 0; p < l && ok; p++) {
            const char c = line[p];
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r') continue;
            if (n == 0) { s5gpu_set_error("%s: %s has sequence in front of its first '>' line", who, fasta_path); ok = 0; break; }
            if (lens[n - 1] == caps[n - 1]) {
                caps[n - 1] = caps[n - 1] ? caps[n - 1] * 2 : 4096;
                char *grown = (char *)realloc(seqs[n - 1], caps[n - 1]);
                if (!grown) { s5gpu_set_error("%s: out of memory", who); ok = 0; break; }
                seqs[n - 1] = grown;
            }
            seqs[n - 1][lens[n - 1]++] = c;
        }
    }
    free(line);
    fclose(f);
    if (ok && n == 0) { s5gpu_set_error("%s: %s holds no '>' line", who, fasta_path); ok = 0; }
    if (ok) h = s5gpu_refseq_build((uint32_t)n, (const char *const *)names, (const char *const *)seqs, lens, model, k, strands, rna, scale, clip);
    for (size_t i = 0; i < n; i++) { free(names[i]); free(seqs[i]); }
    free(names); free(seqs); free(lens); free(caps); free(model);
    return h;
}

/* ---------------------------------------------------------------------------------------------------------------- the handle */
const int16_t *s5gpu_refseq_ref(const void *hv, uint32_t *R_out) {
    const refseq_t *h = (const refseq_t *)hv;
    if (R_out) *R_out = h ? h->R : 0;
    return h ? h->ref : NULL;
}
uint32_t s5gpu_refseq_n_segments(const void *hv) { return hv ? ((const refseq_t *)hv)->n_seg : 0; }
uint32_t s5gpu_refseq_n_contigs(const void *hv) { return hv ? ((const refseq_t *)hv)->n_contigs : 0; }

int s5gpu_refseq_segment(const void *hv, uint32_t i, s5gpu_refseq_segment_t *info) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h || !info || i >= h->n_seg) { s5gpu_set_error("s5gpu_refseq_segment: no segment %u", i); return S5GPU_ERR_ARG; }
    *info = h->seg[i];
    return S5GPU_OK;
}

int s5gpu_refseq_contig(const void *hv, uint32_t i, const char **name_out, uint64_t *len_out, uint32_t *Lk_out) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h || i >= h->n_contigs) { s5gpu_set_error("s5gpu_refseq_contig: no contig %u", i); return S5GPU_ERR_ARG; }
    if (name_out) *name_out = h->names[i];
    if (len_out) *len_out = h->len[i];
    if (Lk_out) *Lk_out = h->Lk[i];
    return S5GPU_OK;
}

int s5gpu_refseq_params(const void *hv, uint32_t *k_out, uint32_t *W_out, int32_t *clip_out) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h) { s5gpu_set_error("s5gpu_refseq_params: NULL handle"); return S5GPU_ERR_ARG; }
    if (k_out) *k_out = h->k;
    if (W_out) *W_out = h->W;
    if (clip_out) *clip_out = h->clip;
    return S5GPU_OK;
}

int s5gpu_refseq_locate(const void *hv, uint32_t col, s5gpu_refseq_loc_t *loc) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h || !loc || col >= h->R) { s5gpu_set_error("s5gpu_refseq_locate: column %u is outside the reference", col); return S5GPU_ERR_ARG; }
    uint32_t lo = 0, hi = h->n_seg - 1;                                    /* the last segment that starts at or before col */
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (h->seg[mid].offset <= col) lo = mid;
        else hi = mid - 1;
    }
    const s5gpu_refseq_segment_t *s = &h->seg[lo];
    const uint32_t p = col - s->offset;
    loc->segment = lo;
    if (p >= s->Lk) { loc->contig = 0xFFFFFFFFu; loc->strand = 0; loc->pos = 0; return S5GPU_REFSEQ_WALL; }
    loc->contig = s->contig; loc->strand = s->strand;
    loc->pos = s->reversed ? s->Lk - 1 - p : p;
    return S5GPU_OK;
}

int s5gpu_refseq_classes(const void *hv, uint32_t *cls_out, uint32_t *K_out) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h) { s5gpu_set_error("s5gpu_refseq_classes: NULL handle"); return S5GPU_ERR_ARG; }
    if (cls_out) memcpy(cls_out, h->cls, sizeof(uint32_t) * h->R);
    if (K_out) *K_out = 1u << (2 * h->k);
    return S5GPU_OK;
}

int s5gpu_refseq_quant(const void *hv, double *mu_out, double *sd_out, double *scale_out) {
    const refseq_t *h = (const refseq_t *)hv;
    if (!h) { s5gpu_set_error("s5gpu_refseq_quant: NULL handle"); return S5GPU_ERR_ARG; }
    if (mu_out) *mu_out = h->mu;
    if (sd_out) *sd_out = h->sd;
    if (scale_out) *scale_out = h->scale;
    return S5GPU_OK;
}

void s5gpu_refseq_close(void *hv) { refseq_free((refseq_t *)hv); }
