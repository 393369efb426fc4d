// dtw_dev.h — what dtw_kernels.hip, dtw_path_kernels.hip, refine_kernels.hip, band_kernels.hip and their host sides share: the quantiser,
// the sDTW cell, a lane's step of the systolic scheme, the packing of a path's decisions and the walk back through them, and, for the device
// only, the wave's side of the scheme (the pieces of a kernel's head, the two walks over the steps, one launch per lane height) and the launchers
// (docs/codecs.md §4.16, §4.17).
// With S5_DTW_HOST defined only the quantiser, the lane code and the path code are declared, as plain C++: tests/test_map.py,
// tests/test_map_second.py, tests/test_align.py and tests/test_refine.py (path_walk_from, §4.20) compile them for the CPU and run the very code a lane runs, 64 lanes in a loop with the lane exchange passed in,
// against the restatement, without a device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/slow5gpu.h"

#ifdef S5_DTW_HOST
#define DTW_HD static inline
#else
#include <hip/hip_runtime.h>

#include <type_traits>
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

// q[0 .. L) of m[0 .. L) read at a stride of `stride` floats, L >= 1: the quantiser of one read, zeros where sd is not usable
DTW_HD void quant_row(const float *m, size_t stride, size_t L, double scale, int32_t clip, int16_t *q) {
    double mu, sd;
    quant_stats(m, stride, L, &mu, &sd);
    const bool ok = quant_ok(sd);
    for (size_t j = 0; j < L; j++) q[j] = ok ? quant_one(m[j * stride], mu, sd, scale, clip) : (int16_t)0;
}

// the rows of a read that count: qlen clamped to the pitch and to QMAX
DTW_HD uint32_t rows_of(uint32_t qlen, uint32_t qpitch) {
    const uint32_t q = qlen < qpitch ? qlen : qpitch;
    return q < QMAX ? q : QMAX;
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

// ---------------------------------------------------------------------------------------------------------------- a lane of k_sdtw2 (§4.19)
// The second-best hit in the same pass.  Column j lies in block j >> bshift.  A lane keeps the least of its row KB in the block it is in, with
// the smallest column that has it, and the four least block minima seen so far, sorted by value, the earlier block first among equals
// (a column tells its block).  Four are enough: the runner-up is the first of them whose block is not within 1 of the first one's, and at
// most three blocks are that near.  Only the lane that holds row Q - 1 is read in the end; an empty entry is (NO_COST, -1).
struct Second {
    uint32_t cur;
    int32_t cur_col;
    uint32_t v[4];
    int32_t c[4];
};
DTW_HD void second_init(Second &S) {
    S.cur = NO_COST; S.cur_col = -1;
    for (int i = 0; i < 4; i++) { S.v[i] = NO_COST; S.c[i] = -1; }
}
// After lane_step at column j, beside lane_best and with its guard (j < R) and its strict <
template <int G, bool WS, int KB>
DTW_HD void lane_second(const Lane<G, WS> &L, Second &S, uint32_t j, uint32_t R) {
    static_assert(KB >= 0 && KB < G, "a row of the lane");
    const uint32_t cand = L.d[KB];
    if (cand < S.cur && j < R) { S.cur = cand; S.cur_col = (int32_t)j; }
}
// When the lane of row Q - 1 has done the last column of a block, or column R - 1: the block's minimum goes into the list (strict <: behind its
// equals; once it is in, the rest moves down one place) and the next block starts empty.  An empty block changes nothing.  Which step that
// is depends on the step and the lane of row Q - 1 alone, so a wave takes it as one scalar branch, every lane with it.
DTW_HD void second_flush(Second &S) {
    uint32_t v = S.cur;
    int32_t c = S.cur_col;
    bool in = false;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        in = in || v < S.v[i];
        const uint32_t tv = S.v[i];
        const int32_t tc = S.c[i];
        S.v[i] = in ? v : tv; S.c[i] = in ? c : tc;
        v = in ? tv : v; c = in ? tc : c;
    }
    S.cur = NO_COST; S.cur_col = -1;
}
// the step at which second_flush is due in a lane that does column j of R: the last column of a block (and, after the walk, once more)
DTW_HD bool second_block_ends(uint32_t j, uint32_t bshift) { const uint32_t mask = (1u << bshift) - 1u; return (j & mask) == mask; }
// mapq: 60 (cost2 - cost) / cost2 in integers, 0 .. 60; 0 without a runner-up or with one of cost 0.  A separation ratio, no probability.
DTW_HD uint32_t second_mapq(uint32_t cost, uint32_t cost2) {
    return cost2 == NO_COST || cost2 == 0u ? 0u : (60u * (cost2 - cost)) / cost2;                      // (cost <= cost2 < 2^26: the product fits)
}
// after the last flush: (cost2, end2, mapq, 0)
DTW_HD U4 second_row(const Second &S, uint32_t bshift) {
    U4 o;
    o.x = NO_COST; o.y = (uint32_t)-1; o.z = 0; o.w = 0;
    if (S.c[0] < 0) return o;
    const int32_t b0 = S.c[0] >> bshift;
    bool found = false;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 1; i < 4; i++) {
        const int32_t b = S.c[i] >> bshift;
        const bool ok = !found && S.c[i] >= 0 && (b >= b0 + 2 || b + 2 <= b0);
        if (ok) { o.x = S.v[i]; o.y = (uint32_t)S.c[i]; }
        found = found || ok;
    }
    o.z = second_mapq(S.v[0], o.x);
    return o;
}

// ---------------------------------------------------------------------------------------------------------------- the path (§4.17)
// The alignment path of a read, walked back through the decisions of the window [start, end] of its row.  A decision is a 2-bit code:
// 0 the diagonal, 1 (i - 1, j), 2 (i, j - 1); 3 does not occur.  A lane's step makes 2 G bits, row k of the lane at bits [2 k, 2 k + 2);
// 16 / G steps fill a 32-bit word, step s of the word at bits [2 G s, 2 G (s + 1)).  A read's words lie [word][lane]: lane l's word w, which
// holds its steps [w 16 / G, (w + 1) 16 / G), is words[w * 64 + l].  At step t lane l does window column t - l.
constexpr uint32_t WMAX = 1u << 20;          // columns of the widest window

// the lane height of a query of Q rows: the smallest G with 64 G >= Q (Q <= QMAX)
DTW_HD uint32_t lane_height(uint32_t Q) { return Q <= 64 ? 1u : Q <= 128 ? 2u : Q <= 256 ? 4u : Q <= 512 ? 8u : 16u; }
// words of a lane that hold `steps` steps, and of the slot of a read of at most qpitch rows and wmax columns (its last lane is 63 at most)
DTW_HD uint32_t path_words(uint32_t G, uint32_t steps) { const uint32_t spw = 16u / G; return (steps + spw - 1) / spw; }
DTW_HD uint32_t path_slot_words(uint32_t qpitch, uint32_t wmax) { return path_words(lane_height(qpitch), wmax + 63u); }

// lane_step without S, yielding the decisions: the same min3 and the same two compares that choose S there
template <int G>
DTW_HD uint32_t lane_step_dirs(Lane<G, false> &L, uint32_t r, uint32_t up) {
    uint32_t dg = L.dg, codes = 0;
    L.dg = up;
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < G; k++) {
        const uint32_t left = L.d[k];
        const uint32_t m = min3u(dg, up, left);
        const uint32_t nd = absdiff(L.q[k], r) + m;
        codes |= (dg == m ? 0u : up == m ? 1u : 2u) << (2 * k);
        dg = left; up = nd;
        L.d[k] = nd;
    }
    return codes;
}
// the codes of step s of a word (s < 16 / G) put into it
DTW_HD uint32_t path_pack(uint32_t word, uint32_t codes, uint32_t s, uint32_t G) { return word | codes << (2u * G * s); }
// cell (i, j) of the window -> the index of the word that holds its code, and the code's shift in it
DTW_HD uint32_t path_cell(uint32_t G, uint32_t i, uint32_t j, uint32_t *shift) {
    const uint32_t l = i / G, k = i - l * G, t = j + l, spw = 16u / G, w = t / spw;
    *shift = 2u * G * (t - w * spw) + 2u * k;
    return w * 64u + l;
}

// Is the row of a read with a query of Q >= 1 rows usable, and its window at most wmax wide?  -> 0 and *W, or the status (*W = 0)
DTW_HD int32_t path_row_check(const U4 &row, uint32_t Q, uint32_t R, uint32_t wmax, uint32_t *W) {
    const int32_t start = (int32_t)row.z, end = (int32_t)row.w;
    *W = 0;
    if (row.y != Q || start < 0 || start > end || (uint32_t)end >= R) return S5GPU_STATUS_PATH_ROW;
    const uint32_t w = (uint32_t)(end - start) + 1u;
    if (w > wmax) return S5GPU_STATUS_PATH_WIDE;
    *W = w;
    return 0;
}

// The walk: from (Q - 1, jend), jend < W, along the decisions to row 0, where it may arrive in any column of the window (§4.20: a window
// wider than the path); that column goes to *start_out.  lo[i], hi[i] (i < Q) get the first and last column of row i, as absolute columns
// (`base` is the window's first).  A decision read from memory chooses the next word, so everything is bounded here: at most Q + W trips;
// i < Q and j < W checked before each use; a word index is clamped to the slot; a code of 3 or a step out of the window ends the walk.
// -> 0, or S5GPU_STATUS_PATH_ROW (*start_out = -1; lo and hi hold a partial path: the caller overwrites them)
DTW_HD int32_t path_walk_from(const uint32_t *words, uint32_t slot_words, uint32_t G, uint32_t Q, uint32_t W, int32_t base, uint32_t jend, int32_t *lo,
                              int32_t *hi, int32_t *start_out) {
    *start_out = -1;
    if (Q == 0 || W == 0 || slot_words == 0 || jend >= W) return S5GPU_STATUS_PATH_ROW;
    const uint32_t top = slot_words * 64u - 1u;
    uint32_t i = Q - 1, j = jend, at = 0xFFFFFFFFu, word = 0;
    hi[i] = base + (int32_t)j;
    for (uint32_t trip = 0; trip < Q + W; trip++) {
        if (i >= Q || j >= W) break;
        if (i == 0) {
            lo[0] = base + (int32_t)j;
            *start_out = base + (int32_t)j;
            return 0;
        }
        uint32_t shift;
        uint32_t x = path_cell(G, i, j, &shift);
        x = x < top ? x : top;
        if (x != at) { word = words[x]; at = x; }                          // (a word holds 16 / G steps of G rows: most moves stay in it)
        const uint32_t code = (word >> shift) & 3u;
        if (code == 3u || (code != 1u && j == 0)) break;
        if (code == 2u) { j--; continue; }
        lo[i] = base + (int32_t)j;
        i--;
        if (code == 0u) j--;
        hi[i] = base + (int32_t)j;
    }
    return S5GPU_STATUS_PATH_ROW;
}
// ... for the window [start, end] of a row of k_sdtw (§4.17), W columns from `start`: from (Q - 1, W - 1), and row 0 has to be reached in
// window column 0.  An arrival right of it is refused after lo[0] was written: like every partial path, the callers overwrite it with -1.
DTW_HD int32_t path_walk(const uint32_t *words, uint32_t slot_words, uint32_t G, uint32_t Q, uint32_t W, int32_t start, int32_t *lo, int32_t *hi) {
    int32_t got;
    const int32_t rc = path_walk_from(words, slot_words, G, Q, W, start, W - 1u, lo, hi, &got);          // (W = 0: jend >= W, refused)
    return rc == 0 && got != start ? S5GPU_STATUS_PATH_ROW : rc;
}

#ifndef S5_DTW_HOST
// lane l <- lane l - 1; lane 0 <- fill.  DPP wave_shr:1 without bound_ctrl: a lane with no source keeps `old`.  One v_mov_b32_dpp, where
// __shfl_up is a ds_bpermute_b32 with its address arithmetic and a select for lane 0.
__device__ __forceinline__ uint32_t shift_up1(uint32_t v, uint32_t fill) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xF, 0xF, false);
}
// ... lane 0 <- 0: with bound_ctrl a lane with no source reads 0, and no register has to be filled first
__device__ __forceinline__ uint32_t shift_up1_zero(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true);
}
// a value that is the same in every lane, as a scalar
__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------------------------------- the wave's side
// What k_sdtw, k_sdtw2, k_sdtw_dirs, k_sdtw_win and k_sdtw_band are made of.  A wave per read, four reads a workgroup: the wave's read ...
__device__ __forceinline__ uint64_t wave_read(uint32_t block_x, uint32_t tid) { return (uint64_t)block_x * 4u + sgpr(tid >> 6); }
// ... and its rows, the same in every lane: every trip count and every branch on Q is the wave's
__device__ __forceinline__ uint32_t wave_rows(uint32_t qlen, uint32_t qpitch) { return sgpr(rows_of(qlen, qpitch)); }
// is a read of Q rows another launch's?  The launch of lane height G takes Q in (32 G, 64 G], that of G = 1 everything up to 64, Q = 0 too
template <int G>
__device__ __forceinline__ bool other_launch(uint32_t Q) { return Q > 64u * G || (G > 1 && Q <= 32u * G); }
// a query value of a lane: row `row` of q, zero at and beyond Q (cells nobody reads).  One value, returned: a helper that fills L.q through
// a reference makes the compiler turn the candidate updates of the walks into chains of selects, 4 to 5 % slower on the device
__device__ __forceinline__ uint32_t query_value(const int16_t *q, uint32_t row, uint32_t Q) { return biased(row < Q ? q[row] : (int16_t)0); }
// kb -> f(std::integral_constant<int, KB>()) for the KB that equals it: a walk is compiled per KB (lane_best), and kb is the same in every
// lane and fixed over a read, so these are scalar branches taken once per read.  f is taken by value: a closure handed down by reference
// keeps what it captured in memory until late in the compilation, which cost 2 % more vector instructions in an inner loop
template <int G, int KB = 0, class F>
__device__ __forceinline__ void with_kb(int kb, F f) {
    if (kb == KB) f(std::integral_constant<int, KB>());
    else if constexpr (KB + 1 < G) with_kb<G, KB + 1>(kb, f);
}

// The steps of one read, the cost family (k_sdtw): lane `last` holds row Q - 1 as its row KB and does column R - 1 at step R - 1 + last
// (R < 2^31).  Every lane steps at every step (FAR): the shifts need every lane, and no step has a branch.  Lane 0 gets the reference value
// by v_readlane from the block of 64 that the wave loads together, zeros behind R.  (k_sdtw2 has a walk of its own, dtw_kernels.hip.)
template <int G, bool WS, int KB>
__device__ __forceinline__ void sdtw_walk(Lane<G, WS> &L, const int16_t *__restrict__ ref, uint32_t R, uint32_t last, uint32_t lane) {
    const uint32_t steps = R + last;
    uint32_t rcur = 0;                                                     // the reference value of the column this lane did last
    uint32_t j = 0u - lane;                                                // the column this lane does next (modulo 2^32 before its column 0)
    auto step = [&](uint32_t rblk, uint32_t k, uint32_t t) {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)rblk, (int)k);
        rcur = shift_up1(rcur, r0);
        const uint32_t up = shift_up1_zero(L.d[G - 1]);
        const int32_t sup = WS ? (int32_t)shift_up1((uint32_t)L.s[G - 1], t + 1) : -1;
        lane_step(L, rcur, up, sup);
        lane_best<G, WS, KB>(L, j, R);
        j++;
    };
    constexpr int UNROLL = G >= 8 ? 2 : 8;                                 // (a step of 16 rows is long enough in itself)
    uint32_t tb = 0;
    for (; tb + 64 <= steps; tb += 64) {
        const uint32_t at = tb + lane;                                     // the wave's block of reference values, zeros behind R
        const uint32_t rblk = biased(at < R ? ref[at] : (int16_t)0);
#pragma unroll UNROLL
        for (uint32_t k = 0; k < 64; k++) step(rblk, k, tb + k);
    }
    if (tb < steps) {
        const uint32_t at = tb + lane;
        const uint32_t rblk = biased(at < R ? ref[at] : (int16_t)0);
        for (uint32_t k = 0; k < steps - tb; k++) step(rblk, k, tb + k);
    }
}

// The steps of one window, the decision family (k_sdtw_dirs; with BEST k_sdtw_win; with BEST and a carry k_sdtw_band): the same lanes and
// shifts over the W columns from ref on, FAR left of the window, zeros behind it.  A lane packs the 2 G bits of 16 / G steps into a word and
// stores it at [word][lane] of the slot (`slot` is the lane's own word 0): the walk steps whole words, nw of them, up to 16 / G - 1 steps
// behind column W - 1 + last, whose codes nobody reads.  BEST: the (cost, end) candidate of the lane's row KB, guarded by j < W.
// A carry (band_kernels.hip) gives lane 0's cell above from the row the tile before left, C.at(x + 1) for window column x, fetched a block of
// 64 columns at a time and handed out by v_readlane as the reference values are, "no cell" behind the window; and lane `wl` (64: none)
// stores its row KB of every column j < W it does with C.store(j, cell).  Without one lane 0's cell above is 0, the free start.
struct NoCarry {};
template <int G, int KB, bool BEST, class CarryT = NoCarry>
__device__ __forceinline__ void dirs_walk(Lane<G, false> &L, const int16_t *__restrict__ ref, uint32_t W, uint32_t nw, uint32_t *slot, uint32_t lane,
                                          const CarryT &C = CarryT(), uint32_t wl = 64u) {
    constexpr bool CARRY = !std::is_same<CarryT, NoCarry>::value;
    constexpr uint32_t SPW = 16 / G, WPB = 64 / SPW;                       // steps per word; words per block of 64 columns
    uint32_t rcur = 0;                                                     // the reference value of the column this lane did last
    uint32_t j = 0u - lane;                                                // the column this lane does next (modulo 2^32 before its column 0)
    for (uint32_t w0 = 0; w0 < nw; w0 += WPB) {
        const uint32_t at = w0 * SPW + lane;                               // the wave's block of columns
        const uint32_t rblk = biased(at < W ? ref[at] : (int16_t)0);
        uint32_t cblk = 0;
        if constexpr (CARRY) cblk = at < W ? C.at(at + 1u) : FAR;
        const uint32_t cnt = nw - w0 < WPB ? nw - w0 : WPB;
        for (uint32_t wi = 0; wi < cnt; wi++) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t s = 0; s < SPW; s++) {
                const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)rblk, (int)(wi * SPW + s));
                rcur = shift_up1(rcur, r0);
                uint32_t up;
                if constexpr (CARRY) up = shift_up1(L.d[G - 1], (uint32_t)__builtin_amdgcn_readlane((int)cblk, (int)(wi * SPW + s)));
                else up = shift_up1_zero(L.d[G - 1]);
                word = path_pack(word, lane_step_dirs(L, rcur, up), s, G);
                if constexpr (BEST) lane_best<G, false, KB>(L, j, W);
                if constexpr (CARRY) { if (lane == wl && j < W) C.store(j, L.d[KB]); }
                j++;
            }
            slot[(uint64_t)(w0 + wi) * 64u] = word;
        }
    }
}
// the words of the walk over W columns of a read or tile whose last row is in lane `last`: it does column W - 1 at step W - 1 + last.
// Clamped to the slot (never less: slot_words holds the widest window + 63 steps of the pitch's G)
template <int G>
__device__ __forceinline__ uint32_t walk_words(uint32_t W, uint32_t last, uint32_t slot_words) {
    const uint32_t nw = path_words(G, W + last);
    return nw < slot_words ? nw : slot_words;
}

// A launch per lane height that a query of at most qpitch rows can need: f(std::integral_constant<int, G>()) for G = 1 and every further G
// with 32 G < qpitch, up to the first that does not return 0.  A wave whose read belongs to another launch returns at once (other_launch).
template <class F>
inline int for_each_lane_height(uint32_t qpitch, F &&f) {
    int rc = f(std::integral_constant<int, 1>());
    if (!rc && qpitch > 64) rc = f(std::integral_constant<int, 2>());
    if (!rc && qpitch > 128) rc = f(std::integral_constant<int, 4>());
    if (!rc && qpitch > 256) rc = f(std::integral_constant<int, 8>());
    if (!rc && qpitch > 512) rc = f(std::integral_constant<int, 16>());
    return rc;
}
// the grid of a kernel with a wave per read and four reads a workgroup of 256
inline dim3 wave_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + 3u) / 4u)); }

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
// k_sdtw over n reads, on st: a launch per lane height that qpitch allows (for_each_lane_height)
int launch_sdtw(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, bool want_start,
                s5gpu_map_row_t *out, hipStream_t st);
// k_sdtw2 likewise: the same rows, and the second-best hit of every read with blocks of 2^bshift columns (6 .. 30)
int launch_sdtw2(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, bool want_start,
                 uint32_t bshift, s5gpu_map_row_t *out, s5gpu_map_second_t *out2, hipStream_t st);
struct PathArgs {
    const int16_t *queries;          // [n, qpitch]
    uint32_t qpitch;
    const uint32_t *qlen;
    const int16_t *ref;
    uint32_t R;
    const U4 *rows;                  // what k_sdtw<G, true> wrote
    uint32_t wmax;
    uint32_t *scratch;               // n slots of slot_words * 64 words
    uint32_t slot_words;
    int32_t *lo, *hi;                // [n, qpitch]
    int32_t *status;
};
// k_sdtw_dirs (a launch per class of lane height) and k_sdtw_trace over n reads, on st; which = 1: the first only, 2: the second only
int launch_path(uint32_t n, const PathArgs &A, hipStream_t st, int which = 3);
// s5gpu_set_option's keys of the path call (dtw_path_api.hip)
int path_set_option(const char *key, long value);
// k_ev_gather: rows [first[i] + skip, ... + qlen[i]) of every read into row i of out [n, qmax], zeros behind
int launch_event_gather(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const uint32_t *qlen, uint32_t skip, uint32_t qmax,
                        s5gpu_event_t *out, hipStream_t st);
#endif

}  // namespace dtwk
