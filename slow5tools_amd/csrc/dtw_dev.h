// dtw_dev.h — what dtw_kernels.hip, dtw_path_kernels.hip and their host sides share: the quantiser, the sDTW cell, a lane's step of the
// systolic scheme, the packing of a path's decisions and the walk back through them, and the launchers (docs/codecs.md §4.16, §4.17).
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

// The walk: from (Q - 1, W - 1) along the decisions to row 0, which it has to reach in window column 0.  lo[i], hi[i] (i < Q) get the first
// and last column of row i, as absolute columns.  A decision read from memory chooses the next word, so everything is bounded here: at
// most Q + W trips; i < Q and j < W checked before each use; a word index is clamped to the slot; a code of 3, a step out of the window or
// an arrival in row 0 right of column 0 ends the walk.  -> 0, or S5GPU_STATUS_PATH_ROW (lo and hi then hold a partial path: the caller
// overwrites them)
DTW_HD int32_t path_walk(const uint32_t *words, uint32_t slot_words, uint32_t G, uint32_t Q, uint32_t W, int32_t start, int32_t *lo, int32_t *hi) {
    if (Q == 0 || W == 0 || slot_words == 0) return S5GPU_STATUS_PATH_ROW;
    const uint32_t top = slot_words * 64u - 1u;
    uint32_t i = Q - 1, j = W - 1, at = 0xFFFFFFFFu, word = 0;
    hi[i] = start + (int32_t)j;
    for (uint32_t trip = 0; trip < Q + W; trip++) {
        if (i >= Q || j >= W) break;
        if (i == 0) {
            if (j != 0) break;
            lo[0] = start;
            return 0;
        }
        uint32_t shift;
        uint32_t x = path_cell(G, i, j, &shift);
        x = x < top ? x : top;
        if (x != at) { word = words[x]; at = x; }                          // (a word holds 16 / G steps of G rows: most moves stay in it)
        const uint32_t code = (word >> shift) & 3u;
        if (code == 3u || (code != 1u && j == 0)) break;
        if (code == 2u) { j--; continue; }
        lo[i] = start + (int32_t)j;
        i--;
        if (code == 0u) j--;
        hi[i] = start + (int32_t)j;
    }
    return S5GPU_STATUS_PATH_ROW;
}

// path_walk's sibling for a window that is wider than the path (§4.20): from (Q - 1, jend), jend < W, to row 0, where it may arrive in any
// column of the window; that column (absolute, as lo and hi: `base` is the window's first) goes to *start_out.  Every bound of path_walk is
// kept: at most Q + W trips; i < Q and j < W checked before each use; a word index clamped to the slot; a code of 3 or a step out of the
// window ends the walk.  -> 0, or S5GPU_STATUS_PATH_ROW (*start_out = -1; lo and hi hold a partial path: the caller overwrites them)
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
        if (x != at) { word = words[x]; at = x; }
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
