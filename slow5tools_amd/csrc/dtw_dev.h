// dtw_dev.h — what dtw_kernels.hip and dtw_api.hip share: the quantiser, the sDTW cell, a lane's step of the systolic scheme and the
// launchers (docs/codecs.md §4.16).
// With S5_DTW_HOST defined only the quantiser and the lane code are declared, as plain C++: tests/test_map.py compiles them for the CPU
// and runs the very code a lane runs, 64 lanes in a loop with the lane exchange passed in, against the restatement, without a device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/slow5gpu.h"

#ifdef S5_DTW_HOST
#define DTW_HD static inline
#else
#include <hip/hip_runtime.h>
#define DTW_HD __host__ __device__ __forceinline__
#endif

// every product and sum of the quantiser is rounded on its own (§4.16: no fused multiply-add); the pragma stands at the head of each
// function that computes in double, so that a translation unit that includes this header keeps its own mode
#ifdef __clang__
#define DTW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DTW_NO_CONTRACT
#endif

namespace dtwk {

constexpr uint32_t QMAX = 1024;              // rows of the largest query: 64 lanes of 16
constexpr uint32_t NO_COST = 0xFFFFFFFFu;    // cost of a read without a query, and of "no candidate yet" (a cell is < 2^26)

struct alignas(16) U4 { uint32_t x, y, z, w; };    // a result row, stored at once

// ---------------------------------------------------------------------------------------------------------------- quant
// mu and sd of m[0 .. L) read at a stride of `stride` floats, L >= 1: double, strictly left to right
DTW_HD void quant_stats(const float *m, size_t stride, size_t L, double *mu_out, double *sd_out) {
    DTW_NO_CONTRACT
    double s = 0.0;
    for (size_t j = 0; j < L; j++) s += (double)m[j * stride];
    const double mu = s / (double)L;
    double v = 0.0;
    for (size_t j = 0; j < L; j++) {
        const double d = (double)m[j * stride] - mu;
        double dd = d * d;
#ifdef __HIP_DEVICE_COMPILE__
        asm volatile("" : "+v"(dd));                               // (the product is a value of its own whatever the contraction mode)
#endif
        v += dd;
    }
    *mu_out = mu;
    *sd_out = sqrt(v / (double)L);
}
// sd of quant_stats usable: otherwise every q is 0
DTW_HD bool quant_ok(double sd) { return sd > 0.0 && sd <= 1.7976931348623157e308; }
// clamp(rint(((x - mu) / sd) * scale), -clip, clip); rint rounds half to even in the default rounding mode
DTW_HD int16_t quant_one(float x, double mu, double sd, double scale, int32_t clip) {
    DTW_NO_CONTRACT
    const double z = ((double)x - mu) / sd;
    const double r = rint(z * scale), c = (double)clip;
    return (int16_t)(int32_t)(r < -c ? -c : r > c ? c : r);
}

// ---------------------------------------------------------------------------------------------------------------- a lane of k_sdtw
// Values are kept biased by 32768, as unsigned: |q - r| is then an unsigned absolute difference (one v_sad_u32 with the add).
DTW_HD uint32_t biased(int16_t v) { return (uint32_t)((int32_t)v + 32768); }
DTW_HD uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
DTW_HD uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; }

// Lane l owns rows [l G, (l + 1) G).  What it keeps between steps: its query values, its cells of the column it did last (d, and their
// starts s with WS), the cell above its first row in that column (dg, sg), and the best of one of its rows so far (lane_best).
template <int G, bool WS>
struct Lane {
    uint32_t q[G];
    uint32_t d[G];
    int32_t s[WS ? G : 1];
    uint32_t dg;
    int32_t sg;
    uint32_t best;
    int32_t best_end, best_start;
};

// "No cell": what stands left of column 0 and on its diagonal.  A lane steps from the wave's first step on, up to l steps before its column
// 0 (and goes on behind column R - 1): there it adds to FAR, at most 65535 a cell and 64 steps, so what it holds at column 0 is still above
// every cell of the matrix (< 2^26) and far below 2^32, and min3 takes the cell from above, the only real one.  No step needs a predicate.
constexpr uint32_t FAR = 1u << 30;

// before the first step.  Lane 0 has no row above it: there the cell above (what the wave shift fills in) and dg stand for "a path starts
// here", cost 0, and sg for the column it starts in.
template <int G, bool WS>
DTW_HD void lane_init(Lane<G, WS> &L, bool top) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < G; k++) { L.d[k] = FAR; if (WS) L.s[k] = -1; }
    L.dg = top ? 0u : FAR;
    L.sg = top ? 0 : -1;
    L.best = NO_COST; L.best_end = -1; L.best_start = -1;
}

// One column of the lane's rows.  r: the reference value of the column (biased); up / sup: the cell of the row above the lane's first in
// this column.  Lane 0 is given up = 0 and sup = the NEXT column's index: its row 0 then has dg = up = 0 in every column, takes the
// diagonal, and finds the column's own index in sg.  The same code in every lane, no branch.
// The predecessor of least D is chosen, ties to the diagonal, then (i - 1, j), then (i, j - 1).
template <int G, bool WS>
DTW_HD void lane_step(Lane<G, WS> &L, uint32_t r, uint32_t up, int32_t sup) {
    uint32_t dg = L.dg;
    int32_t sg = L.sg;
    L.dg = up;
    L.sg = sup;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < G; k++) {
        const uint32_t left = L.d[k];
        const uint32_t m = min3u(dg, up, left);
        const uint32_t nd = absdiff(L.q[k], r) + m;
        int32_t ns = -1;
        if (WS) {
            const int32_t sl = L.s[k];
            ns = dg == m ? sg : up == m ? sup : sl;
            sg = sl; L.s[k] = ns;
        }
        dg = left; up = nd; sup = ns;
        L.d[k] = nd;
    }
}

// After lane_step at column j (as the lane counts, modulo 2^32: "below 0" before its column 0): the cell of the lane's row KB is a
// candidate for (cost, end) where j < R.  Strict <: the smallest j wins.  KB is the same in every lane of a wave and fixed over a read, so
// the walk is compiled per KB and no step pays for the choice.  Every lane keeps its own best; only the lane that holds row Q - 1 is read
// in the end.
template <int G, bool WS, int KB>
DTW_HD void lane_best(Lane<G, WS> &L, uint32_t j, uint32_t R) {
    static_assert(KB >= 0 && KB < G, "a row of the lane");
    const uint32_t cand = L.d[KB];
    if (cand < L.best && j < R) { L.best = cand; L.best_end = (int32_t)j; L.best_start = WS ? L.s[KB] : -1; }
}

DTW_HD U4 result_row(uint32_t cost, uint32_t qlen, int32_t start, int32_t end) {
    U4 o;
    o.x = cost; o.y = qlen; o.z = (uint32_t)start; o.w = (uint32_t)end;
    return o;
}

#ifndef S5_DTW_HOST
struct QueryArgs {
    const s5gpu_event_t *rows;
    const uint64_t *first;           // n + 1
    const int32_t *ev_status;        // may be nullptr: every read 0
    uint32_t skip, qmax, qmin;
    double scale;
    int32_t clip;
    int16_t *queries;                // [n, qmax]
    uint32_t *qlen;
    int32_t *status;
};
// k_ev_query over n reads, on st
int launch_queries(uint32_t n, const QueryArgs &A, hipStream_t st);
// k_sdtw over n reads, on st: a launch per class of lane height that qpitch allows
int launch_sdtw(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, bool want_start,
                s5gpu_map_row_t *out, hipStream_t st);
#endif

}  // namespace dtwk
