// refine_dev.h — what refine_kernels.hip and refine_api.hip share (docs/codecs.md §4.20): the sums of a path row, the solve, the
// requantiser, the window around a row, and the launchers.  With S5_REFINE_HOST (or S5_DTW_HOST) defined only the plain C++ is declared
// (the switch of dtw_dev.h and pileup_dev.h): tests/test_refine.py compiles it for the CPU and runs the very code a lane runs against the
// restatement, without a device.  Further down: the same for whole reads (§4.24), on the ragged layout and the segments of ragged_dev.h;
// tests/test_extend_refine.py compiles that part behind S5_PILEUP_HOST.
#pragma once
#if (defined(S5_REFINE_HOST) || defined(S5_PILEUP_HOST)) && !defined(S5_DTW_HOST)
#define S5_DTW_HOST
#endif
#if defined(S5_DTW_HOST) && !defined(S5_PILEUP_HOST)
#define S5_PILEUP_HOST
#endif
#include "dtw_dev.h"
#include "pileup_dev.h"
#include "band_dev.h"

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

// ---------------------------------------------------------------------------------------------------------------- whole reads (§4.24)
// The fit along the ragged paths of extend (the layout, the verdicts and the segments of ragged_dev.h, §4.22, with ev_skip = 0), and the
// bookkeeping of the rounds of s5gpu_extend_refine_dev.  There is no wmax: a row of a path that passed pilek::row_ok in every row has
// hi - lo + 1 <= R trips, and j < R is checked again before ref[j] is read (row_sums with R for wmax).  A read has fewer than 2^20 + 2^26
// cells and each term is below 2^30: every sum is below 2^57.

// Rows r0 + lane, r0 + lane + step, ... < r1 of a read whose lo, hi and q point at ITS row 0, added to S (pilek::seg_cells' walk)
DTW_HD void seg_sums(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, const int16_t *q, const int16_t *ref,
                     uint32_t R, Sums &S) {
    for (uint32_t i = r0 + lane; i < r1; i += step) row_sums(lo[i], hi[i], (int32_t)q[i], ref, R, R, S);
}
DTW_HD void sums_add(Sums &d, const Sums &s) { d.n += s.n; d.sq += s.sq; d.sr += s.sr; d.sqq += s.sqq; d.sqr += s.sqr; d.srr += s.srr; }

// The verdict of §4.22 and the sums of a read -> its fit and its status: a skipped read keeps the status that came in (0 for one without a
// query), a bad one has S5GPU_STATUS_PATH_ROW, both without a fit; a used one has fit_solve's status, and the sums whatever that is.
DTW_HD int32_t long_fit_status(uint32_t verdict, int32_t status_in, const Sums &S, const s5gpu_refine_params_t &P, s5gpu_fit_t *F) {
    *F = fit_none();
    if (verdict & pilek::V_SKIPPED) return status_in;
    if (verdict & pilek::V_BAD) return S5GPU_STATUS_PATH_ROW;
    const int32_t st = fit_solve(S, P, &F->a, &F->b);
    F->n = S.n; F->sq = S.sq; F->sr = S.sr; F->sqq = S.sqq; F->sqr = S.sqr; F->srr = S.srr;
    return st;
}

// What a read does in a round, and the status it has behind it (*st).  Modes: 0 nothing (it keeps what it has), 1 copies of what came in,
// 2 the trial round becomes its result, 3 no result at all.  Round 0: verdict is that of the path that came in and cur the status that came
// in.  Round k >= 1: cur is the status the read has, sf the fit's and sw the band's status of the trial; a read with a status or without a
// query takes no part any more.
DTW_HD int long_round_rule(uint32_t round, uint32_t verdict, uint32_t Q, int32_t cur, int32_t sf, int32_t sw, int32_t *st) {
    if (round == 0) {
        *st = verdict & pilek::V_SKIPPED ? cur : verdict & pilek::V_BAD ? S5GPU_STATUS_PATH_ROW : 0;
        return verdict == pilek::V_USED ? 1 : 3;
    }
    *st = cur;
    if (cur != 0 || Q == 0) return 0;
    *st = sf ? sf : sw;
    return *st == 0 ? 2 : sf == S5GPU_STATUS_PATH_ROW ? 3 : 0;
}
// the row of a read behind a round: rows_in / the trial's row / the row it has with its new status / the row of no result
DTW_HD s5gpu_ext_row_t long_round_row(int mode, int32_t st, const s5gpu_ext_row_t &from, const s5gpu_ext_row_t &has) {
    if (mode == 1 || mode == 2) return from;
    if (mode == 3) return bandk::row_none(st);
    s5gpu_ext_row_t r = has;
    r.status = st;
    return r;
}

// the work area of s5gpu_path_fit_long_dev: that of a ragged pileup call (the sort's part is not used), then the reads' sums
struct FitLongWork { uint64_t o_sums, bytes; };
DTW_HD FitLongWork fit_long_work(uint32_t n, uint64_t total_rows) {
    FitLongWork w;
    w.o_sums = pilek::long_work(n, total_rows).bytes;
    w.bytes = w.o_sums + pilek::up16(sizeof(Sums) * (uint64_t)(n ? n : 1u));
    return w;
}
// ... and of s5gpu_extend_refine_dev: the fit's, then a trial round (rows, fits, the fit's statuses, the two status arrays the rounds
// alternate between, lo, hi and the query)
struct RefineLongWork { uint64_t o_rows, o_fit, o_sf, o_st0, o_st1, o_lo, o_hi, o_q, bytes; };
DTW_HD RefineLongWork refine_long_work(uint32_t n, uint64_t total_rows) {
    RefineLongWork w;
    const uint64_t m = n ? n : 1u, s4 = pilek::up16(4u * m), t = total_rows ? total_rows : 1u;
    w.o_rows = fit_long_work(n, total_rows).bytes;
    w.o_fit = w.o_rows + 32u * m; w.o_sf = w.o_fit + 64u * m; w.o_st0 = w.o_sf + s4; w.o_st1 = w.o_st0 + s4; w.o_lo = w.o_st1 + s4;
    w.o_hi = w.o_lo + pilek::up16(4u * t); w.o_q = w.o_hi + pilek::up16(4u * t); w.bytes = w.o_q + pilek::up16(2u * t);
    return w;
}

#ifndef S5_DTW_HOST
// the fit over ragged paths: A.status is status_in, A.events and A.acc are not used, A.ev_skip is 0, A.work has fit_long_work().bytes
struct FitLongArgs {
    pilek::PileLongArgs A;
    s5gpu_refine_params_t P;
    s5gpu_fit_t *fit;                // [n]
    int16_t *queries_out;            // [total_rows], or nullptr: q' at the rows of the reads whose status_out is 0, nothing else is written
    int32_t *status_out;             // [n]
};
// the bookkeeping of a round over the verdicts and segments the last launch_long_verdicts / launch_fit_long left in A.work
struct RoundLongArgs {
    pilek::PileLongArgs A;           // queries, lo, hi, status: what came in (round 0 reads them)
    const s5gpu_ext_row_t *rows_in;
    const int16_t *t_q;
    const s5gpu_ext_row_t *t_rows;
    const int32_t *t_lo, *t_hi;
    const s5gpu_fit_t *t_fit;
    const int32_t *t_sf;
    const int32_t *cur_in;           // the statuses the reads have (round 0: those that came in) ...
    int32_t *cur_out;                // ... and have behind this round: another array
    int16_t *q;
    s5gpu_ext_row_t *rows;
    int32_t *lo, *hi;
    s5gpu_fit_t *fit;
    uint32_t *rounds;
};
// The launchers of refine_long_kernels.hip.  launch_long_verdicts: pilek::launch_long_plan_check (k_pileup_long_plan and k_pileup_long_check, no sort) over the
// reads of A: the verdicts and the segments' prefix in A.work
int launch_long_verdicts(const pilek::PileLongArgs &A, hipStream_t st);
// ... then k_path_fit_long, k_fit_long_solve and (queries_out) k_requant_long
int launch_fit_long(const FitLongArgs &F, hipStream_t st);
// k_refine_long_gate: st[k] = rows[k].status
int launch_gate_long(uint32_t n, const s5gpu_ext_row_t *rows, int32_t *st_out, hipStream_t st);
// k_refine_long_round
int launch_round_long(const RoundLongArgs &B, uint32_t round, hipStream_t st);
// which of these the calls launch: "refine_long_passes", the one key of s5gpu_set_option here
uint32_t long_passes();
int long_set_option(const char *key, long value);
#endif

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
