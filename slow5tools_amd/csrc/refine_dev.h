// refine_dev.h — what refine_kernels.hip and refine_api.hip share (docs/codecs.md §4.20): the sums of a path row, the solve, the
// requantiser, the window around a row, and the launchers.  With S5_REFINE_HOST (or S5_DTW_HOST) defined only the plain C++ is declared
// (the switch of dtw_dev.h and pileup_dev.h): tests/test_refine.py compiles it for the CPU and runs the very code a lane runs against the
// restatement, without a device.
#pragma once
#if defined(S5_REFINE_HOST) && !defined(S5_DTW_HOST)
#define S5_DTW_HOST
#endif
#if defined(S5_DTW_HOST) && !defined(S5_PILEUP_HOST)
#define S5_PILEUP_HOST
#endif
#include "dtw_dev.h"
#include "pileup_dev.h"

namespace refk {

using dtwk::U4;

constexpr uint32_t PAD_MAX = 65535, ITERS_MAX = 4;
static_assert(sizeof(s5gpu_fit_t) == 64 && sizeof(s5gpu_refine_params_t) == 40, "include/slow5gpu.h fixes these layouts");

// the six sums of §4.20, exact: at most 1024 + 2^20 cells, each term below 2^30
struct Sums { int64_t n, sq, sr, sqq, sqr, srr; };

// every parameter inside the ranges of §4.20 (NaN fails every compare)
DTW_HD bool params_ok(const s5gpu_refine_params_t &P) {
    const double big = 1.7976931348623157e308;
    return P.a_min > 0.0 && P.a_min <= P.a_max && P.a_max <= big && P.b_max >= 0.0 && P.b_max <= big && P.clip >= 1 && P.clip <= 32767 &&
           P.pad <= PAD_MAX && P.min_cells >= 2u && P.iters >= 1u && P.iters <= ITERS_MAX;
}

// The cells of one row of a path that passed pilek::row_ok in EVERY row and spans at most wmax columns: columns lo .. hi, at most wmax
// trips, j < R checked again before ref[j] is read.  q: the row's query value.
DTW_HD void row_sums(int32_t lo, int32_t hi, int32_t q, const int16_t *ref, uint32_t R, uint32_t wmax, Sums &S) {
    const uint32_t trips = (uint32_t)(hi - lo) + 1u;
    uint32_t j = (uint32_t)lo;
    int64_t cnt = 0, sr = 0, srr = 0;
    for (uint32_t t = 0; t < trips && t < wmax && j < R; t++, j++) {
        const int64_t r = (int64_t)ref[j];
        sr += r; srr += r * r; cnt++;
    }
    const int64_t q64 = (int64_t)q;
    S.n += cnt; S.sq += cnt * q64; S.sqq += cnt * q64 * q64;
    S.sr += sr; S.sqr += q64 * sr; S.srr += srr;
}

// The least-squares line r = a q + b in double, every operation rounded on its own, the products before the subtraction (§4.20).
// -> 0 and a, b; or S5GPU_STATUS_FIT_FLAT / S5GPU_STATUS_FIT_RANGE and a = 1, b = 0
DTW_HD int32_t fit_solve(const Sums &S, const s5gpu_refine_params_t &P, double *a_out, double *b_out) {
    DTW_NO_CONTRACT
    *a_out = 1.0; *b_out = 0.0;
    const double n = (double)S.n, sq = (double)S.sq, sr = (double)S.sr, sqq = (double)S.sqq, sqr = (double)S.sqr;
    const double nqq = n * sqq, qq = sq * sq;
    const double den = nqq - qq;
    if (S.n < (int64_t)P.min_cells || !(den > 0.0)) return S5GPU_STATUS_FIT_FLAT;
    const double nqr = n * sqr, qr = sq * sr;
    const double a = (nqr - qr) / den;
    const double aq = a * sq;
    const double b = (sr - aq) / n;
    const double big = 1.7976931348623157e308;
    const bool a_ok = a >= P.a_min && a <= P.a_max && a <= big;            // (NaN fails the compares)
    const bool b_ok = (b < 0.0 ? -b : b) <= P.b_max;
    if (!a_ok || !b_ok) return S5GPU_STATUS_FIT_RANGE;
    *a_out = a; *b_out = b;
    return 0;
}

// clamp(rint(a q0 + b), -clip, clip): the product is rounded, then the sum; rint rounds half to even (a and b are finite)
DTW_HD int16_t requant_one(int16_t q0, double a, double b, int32_t clip) {
    DTW_NO_CONTRACT
    const double p = a * (double)q0;
    const double s = p + b;
    const double r = rint(s), c = (double)clip;
    return (int16_t)(int32_t)(r < -c ? -c : r > c ? c : r);
}

// The window around the row of a read with a query of Q >= 1 rows: the row's rules of dtwk::path_row_check, then ws = max(0, start - pad),
// we = min(R - 1, end + pad), W = we - ws + 1 <= wmax.  -> 0 with *ws and *W, or the status (*ws = *W = 0)
DTW_HD int32_t win_row_check(const U4 &row, uint32_t Q, uint32_t R, uint32_t pad, uint32_t wmax, uint32_t *ws, uint32_t *W) {
    const int32_t start = (int32_t)row.z, end = (int32_t)row.w;
    *ws = 0; *W = 0;
    if (row.y != Q || start < 0 || start > end || (uint32_t)end >= R) return S5GPU_STATUS_PATH_ROW;
    const uint32_t s = (uint32_t)start > pad ? (uint32_t)start - pad : 0u;
    const uint64_t e64 = (uint64_t)(uint32_t)end + pad;
    const uint32_t e = e64 < (uint64_t)(R - 1u) ? (uint32_t)e64 : R - 1u;
    const uint32_t w = e - s + 1u;
    if (w > wmax) return S5GPU_STATUS_PATH_WIDE;
    *ws = s; *W = w;
    return 0;
}

// the fit of a read that was not fitted
DTW_HD s5gpu_fit_t fit_none() {
    s5gpu_fit_t f;
    f.a = 1.0; f.b = 0.0; f.n = 0; f.sq = 0; f.sr = 0; f.sqq = 0; f.sqr = 0; f.srr = 0;
    return f;
}

#ifndef S5_DTW_HOST
struct FitArgs {
    const int16_t *queries;          // [n, qpitch]
    uint32_t qpitch;
    const uint32_t *qlen;
    const int16_t *ref;
    uint32_t R;
    const int32_t *lo, *hi;          // [n, qpitch]
    const int32_t *status_in;
    uint32_t wmax;
    s5gpu_refine_params_t P;
    s5gpu_fit_t *fit;
    int16_t *queries_out;            // [n, qpitch], or nullptr
    int32_t *status_out;
};
struct WinArgs {
    const int16_t *queries;          // [n, qpitch]
    uint32_t qpitch;
    const uint32_t *qlen;
    const int16_t *ref;
    uint32_t R;
    const U4 *rows_in;
    const int32_t *gate;             // nullptr, or a status per read: not 0 -> the read is passed over and has this status
    uint32_t pad, wmax;
    uint32_t *scratch;               // n slots of slot_words * 64 words
    uint32_t slot_words;
    U4 *rows_out;
    int32_t *lo, *hi;                // [n, qpitch]
    int32_t *status;
};
// what a round of s5gpu_refine_dev tries (t_*), and what the call gives back (the rest)
struct RoundArgs {
    uint32_t qpitch;
    const uint32_t *qlen;
    const int16_t *q_in;
    const U4 *rows_in;
    const int32_t *lo_in, *hi_in, *status_in;
    const int16_t *t_q;
    const U4 *t_rows;
    const int32_t *t_lo, *t_hi;
    const s5gpu_fit_t *t_fit;
    const int32_t *t_st_fit, *t_st_win;
    int16_t *q;
    U4 *rows;
    int32_t *lo, *hi;
    s5gpu_fit_t *fit;
    int32_t *status;
    uint32_t *rounds;
};
// k_path_fit over n reads, on st
int launch_fit(uint32_t n, const FitArgs &A, hipStream_t st);
// k_sdtw_win (a launch per class of lane height) and k_sdtw_trace_win over n reads, on st
int launch_window(uint32_t n, const WinArgs &A, hipStream_t st);
// k_refine_round over n reads, on st: round 0 writes the outputs from what came in, round k >= 1 takes a trial round over where it succeeded
int launch_round(uint32_t n, const RoundArgs &A, uint32_t round, hipStream_t st);
#endif

}  // namespace refk
