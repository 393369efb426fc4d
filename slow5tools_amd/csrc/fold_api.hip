// fold_api.hip — host side of the fold calls (include/slow5gpu.h, "model"; docs/codecs.md §4.26): the argument checks and launches of the
// two device entry points, the fold a handle makes when it is closed folded (pileup_api.hip and contrast_api.hip call it), and the estimate
// of a level table from a folded table, which is host arithmetic in double and has this one definition.
#include <math.h>

#include "pileup_host.h"
#include "fold_dev.h"

namespace {

bool fold_args_ok(const char *who, const void *in, uint32_t R, const uint32_t *cls, uint32_t K, void *out, uint32_t most, const char *most_txt) {
    if (R == 0 || R > most || K == 0 || K > most) { s5gpu_set_error("%s: %u columns onto %u classes (1 .. %s each)", who, R, K, most_txt); return false; }
    if (!in || !cls || !out) { s5gpu_set_error("%s: NULL argument", who); return false; }
    if (((uintptr_t)in & 15u) || ((uintptr_t)out & 15u) || ((uintptr_t)cls & 3u)) { s5gpu_set_error("%s: misaligned argument (in, out: 16 bytes; cls: 4)", who); return false; }
    if (in == out) { s5gpu_set_error("%s: the output is the input", who); return false; }
    return true;
}

}  // namespace

int pilek::fold_checked(const char *who, const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, hipStream_t st) {
    if (!fold_args_ok(who, acc_in, R, cls, K, acc_out, RMAX, "2^26")) return S5GPU_ERR_ARG;
    return launch_fold(acc_in, R, cls, K, acc_out, st);
}

int pilek::hist_fold_checked(const char *who, const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, hipStream_t st) {
    if (!fold_args_ok(who, hist_in, R, cls, K, hist_out, HIST_RMAX, "2^22")) return S5GPU_ERR_ARG;
    return launch_hist_fold(hist_in, R, cls, K, hist_out, st);
}

extern "C" int s5gpu_pileup_fold_dev(const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, void *stream) {
    return pilek::fold_checked("s5gpu_pileup_fold_dev", acc_in, R, cls, K, acc_out, (hipStream_t)stream);
}

extern "C" int s5gpu_pile_hist_fold_dev(const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, void *stream) {
    return pilek::hist_fold_checked("s5gpu_pile_hist_fold_dev", hist_in, R, cls, K, hist_out, (hipStream_t)stream);
}

extern "C" int s5gpu_quant_stats_host(const float *m, size_t L, double *mu_out, double *sd_out) {
    if (!m || !mu_out || !sd_out || L == 0) { s5gpu_set_error("s5gpu_quant_stats_host: NULL argument or no value"); return S5GPU_ERR_ARG; }
    dtwk::quant_stats(m, 1, L, mu_out, sd_out);
    return S5GPU_OK;
}

extern "C" int s5gpu_kmer_model_solve(const void *acc_folded, uint32_t K, double mu, double sd, double scale, uint32_t min_cells, const float *levels_in,
                                      s5gpu_kmer_row_t *rows_out) {
    DTW_NO_CONTRACT
    const char *who = "s5gpu_kmer_model_solve";
    if (!acc_folded || !levels_in || !rows_out || K == 0) { s5gpu_set_error("%s: NULL argument or no class", who); return S5GPU_ERR_ARG; }
    if (!dtwk::quant_ok(sd) || !dtwk::quant_ok(scale)) { s5gpu_set_error("%s: sd and scale have to be finite and above 0", who); return S5GPU_ERR_ARG; }
    s5gpu_pile_total_t T;
    memcpy(&T, acc_folded, sizeof T);
    if (T.R != K) { s5gpu_set_error("%s: a table of %u columns, K = %u", who, T.R, K); return S5GPU_ERR_ARG; }
    const uint8_t *cols = (const uint8_t *)acc_folded + sizeof T;
    const double unit = sd / scale;
    for (uint32_t c = 0; c < K; c++) {
        s5gpu_pile_col_t col;
        memcpy(&col, cols + sizeof col * (size_t)c, sizeof col);
        s5gpu_kmer_row_t r;
        memset(&r, 0, sizeof r);
        r.cells = col.n_events;
        if (col.n_events == 0 || col.n_events < min_cells) {
            r.level = (double)levels_in[c];
            r.kept = 1;
        } else {
            const double n = (double)col.n_events;
            const double mean_q = (double)col.sum_q / n;
            const double msq = (double)col.sumsq_q / n;
            const double sq = mean_q * mean_q;
            const double var_q = msq - sq > 0.0 ? msq - sq : 0.0;
            const double um = unit * mean_q;
            r.level = mu + um;
            r.stdv = unit * sqrt(var_q);
            r.dwell = (double)col.n_samples / n;
        }
        rows_out[c] = r;
    }
    return S5GPU_OK;
}
