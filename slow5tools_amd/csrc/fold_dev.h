// fold_dev.h — what fold_kernels.hip and fold_api.hip share (docs/codecs.md §4.26): the fold of a table of pileup (§4.18) and of a level
// histogram (§4.23) onto classes.  cls[j] is the class of input column j; the column is kept iff cls[j] < K, and every member of output
// column c is the sum (min_q, max_q: the minimum, the maximum) over the kept, non-empty j with cls[j] = c.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of pileup_dev.h): tests/test_fold.py compiles it for the CPU and
// runs the very code a lane runs, with plain adds in place of the atomics, against the restatement.
#pragma once
#include "pileup_dev.h"

namespace pilek {

constexpr uint32_t FOLD_LDS_K = MAX_COLS;    // the most classes a workgroup keeps in LDS: 48 KB
constexpr uint64_t FOLD_CELLS_MAX = (uint64_t)1 << 32;   // an input of this many cells or more is refused: depth, n_events and the bins are 32-bit

// May this call add at all?  cells: the input head's total; r_in, r_out: the R the two heads hold, against the call's R and K
PILE_HD bool fold_heads_ok(uint64_t cells, uint32_t r_in, uint32_t R, uint32_t r_out, uint32_t K) { return cells < FOLD_CELLS_MAX && r_in == R && r_out == K; }
// ... and for histograms: words 9 .. 11 of the two heads (q0, shift, bins)
PILE_HD bool fold_hist_heads_ok(const uint32_t *hin, const uint32_t *hout) { return hin[9] == hout[9] && hin[10] == hout[10] && hin[11] == HIST_BINS && hout[11] == HIST_BINS; }

// Input column `in` of class cls merged into its class: into the window's table where the class lies inside (W.lo = 0 and W.cols >= K,
// or W.cols = 0: no window), else into the table of K columns.  A class indexes either only behind cls < K.  A dropped or an empty column
// adds nothing, so the 32767 / -32768 pair of an empty column does not leak.  cells / cost: the caller's running totals of what it kept.
template <class Ops>
PILE_HD void fold_col(const s5gpu_pile_col_t &in, uint32_t cls, uint32_t K, const Window &W, s5gpu_pile_col_t *win, s5gpu_pile_col_t *table, uint64_t *cells,
                      uint64_t *cost) {
    if (cls >= K || in.n_events == 0) return;
    s5gpu_pile_col_t c = in;                                               // (col_merge empties its source: a copy)
    *cells += c.n_events;
    *cost += c.sum_cost;
    uint32_t slot;
    if (window_slot(W, cls, &slot) && slot < K) col_merge<Ops>(win + slot, &c);
    else col_merge<Ops>(table + cls, &c);
}

// Bin `bin` of a kept column of a histogram: v, its count.  -> what it adds to the caller's cells
template <class Ops>
PILE_HD uint64_t fold_bin(uint32_t v, uint32_t cls, uint32_t K, uint32_t bin, uint32_t *table) {
    if (cls >= K || v == 0u) return 0;
    Ops::add32(table + (uint64_t)cls * HIST_BINS + (bin & (HIST_BINS - 1u)), v);
    return v;
}

#ifndef S5_PILEUP_HOST
// k_pile_fold and k_pile_hist_fold on st (fold_kernels.hip); the arguments are checked by the callers (fold_api.hip)
int launch_fold(const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, hipStream_t st);
int launch_hist_fold(const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, hipStream_t st);
int fold_set_option(const char *key, long value);
// the checks of s5gpu_pileup_fold_dev and s5gpu_pile_hist_fold_dev (who names the caller), then the launch
int fold_checked(const char *who, const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, hipStream_t st);
int hist_fold_checked(const char *who, const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, hipStream_t st);
#endif

}  // namespace pilek
