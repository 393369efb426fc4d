// refine_kernels.hip — per-read level rescaling from the path, and a windowed realign, on the device (docs/codecs.md §4.20):
//   k_path_fit        : a wave per read, four reads a workgroup (the shape of k_pileup).  The wave validates the WHOLE path (each lane its rows
//                       i = lane, lane + 64, ..., one vote), then the lanes sum their rows' cells, the six int64 sums are reduced across the
//                       wave, the line is solved, a and b are made wave-uniform, and each lane writes its rows of q'; lane 0 writes the fit.
//   k_sdtw_win<G>     : the systolic wave of k_sdtw_dirs over the read's own window ref + ws of W' columns (dirs_walk of dtw_dev.h with
//                       BEST); in the same pass it carries the (cost, end) candidate of k_sdtw: lane_best on the lane that holds row Q - 1,
//                       compiled per KB, guarded by j < W'.  No S.  It writes the decision words in the slot layout of §4.17 and the row
//                       (cost', qlen, -1, end').
//   k_sdtw_trace_win  : a SEPARATE launch (the kernel boundary makes the words visible), a lane per read: path_walk_from from
//                       (Q - 1, end' - ws) to wherever it arrives in row 0; that column is start', written into the row.
//   k_refine_round    : the bookkeeping of s5gpu_refine_dev between rounds: a trial round is taken over where it succeeded.
// Values read from memory form addresses here (lo, hi, the rows, the decision words).  The rules, those of §4.17 / §4.18:
//   1. trip counts come from qlen, the rows and wmax only, checked before any loop: Q is qlen clamped to the pitch and to 1024; a row of a
//      path has hi - lo + 1 <= wmax trips once the whole path passed row_ok and its span is <= wmax; a window has W' <= wmax columns
//      (win_row_check, in BOTH window kernels); the walk has at most Q + W' trips;
//   2. k_path_fit reads ref[j] behind j < R, established by the validation and checked again in row_sums; k_sdtw_win reads ref[ws + x] for
//      x < W' only (ws + W' - 1 <= R - 1) and writes the words [0, min(words of its steps, slot_words)) of its own slot;
//   3. k_sdtw_trace_win: i < Q and j < W' before each use, the word index clamped to the slot, a code of 3 or a step out of the window
//      ends the walk with S5GPU_STATUS_PATH_ROW and -1s (path_walk_from, dtw_dev.h); it does not trust the end' the pass before wrote;
//   4. early returns are wave-uniform; a wave shares nothing but shifts, votes and shuffles that every lane executes: no barrier, no LDS;
//   5. vector stores and HIP builtins only.
#include "dev_common.h"
#include "refine_dev.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace dtwk;
using namespace refk;

namespace {

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// lane 0's value in every lane, as a scalar
__device__ __forceinline__ double wave_first(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __longlong_as_double((long long)((uint64_t)lo | ((uint64_t)hi << 32)));
}

}  // namespace

__global__ __launch_bounds__(256) void k_path_fit(uint32_t n, FitArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;                                                // (the wave's branch)
    const uint32_t Q = wave_rows(A.qlen[read], A.qpitch);
    int32_t st = __builtin_amdgcn_readfirstlane(A.status_in[read]);
    const int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
    const int16_t *q = A.queries + read * A.qpitch;
    bool path = st == 0 && Q != 0;
    if (path) {                                                           // (wave-uniform)
        bool ok = true;
        for (uint32_t i = lane; i < Q; i += 64u) ok = ok && pilek::row_ok(i, lo[i], hi[i], i ? hi[i - 1] : 0, A.R);
        if (!__all(ok ? 1 : 0)) st = S5GPU_STATUS_PATH_ROW;               // one vote: the whole path or nothing of it
        else if ((int64_t)hi[Q - 1] - (int64_t)lo[0] + 1 > (int64_t)A.wmax) st = S5GPU_STATUS_PATH_WIDE;
        st = __builtin_amdgcn_readfirstlane(st);
        path = st == 0;
    }
    s5gpu_fit_t F = fit_none();
    if (path) {
        Sums S = {0, 0, 0, 0, 0, 0};
        for (uint32_t i = lane; i < Q; i += 64u) row_sums(lo[i], hi[i], (int32_t)q[i], A.ref, A.R, A.wmax, S);
        S.n = wave_sum(S.n); S.sq = wave_sum(S.sq); S.sr = wave_sum(S.sr);
        S.sqq = wave_sum(S.sqq); S.sqr = wave_sum(S.sqr); S.srr = wave_sum(S.srr);
        double a, b;
        st = __builtin_amdgcn_readfirstlane(fit_solve(S, A.P, &a, &b));   // (every lane holds the same sums: the solve is one SIMD pass)
        F.a = wave_first(a); F.b = wave_first(b);
        F.n = S.n; F.sq = S.sq; F.sr = S.sr; F.sqq = S.sqq; F.sqr = S.sqr; F.srr = S.srr;
    }
    if (A.queries_out) {
        int16_t *qo = A.queries_out + read * A.qpitch;
        for (uint32_t x = lane; x < A.qpitch; x += 64u) {
            int16_t v = 0;
            if (path && x < Q) v = st == 0 ? requant_one(q[x], F.a, F.b, A.P.clip) : q[x];
            qo[x] = v;
        }
    }
    if (lane == 0) {
        A.fit[read] = F;
        A.status_out[read] = st;
    }
}

// kb -> the walk compiled for it.  The kernel's own dispatch, as k_sdtw_band's TileWalk, not with_kb of dtw_dev.h: through the closure the
// window call measured 0.5 to 1 % slower; with this struct the kernel has the instruction counts it had with a walk of its own
template <int G, int KB = 0>
struct WinWalk {
    static __device__ __forceinline__ void run(int kb, Lane<G, false> &L, const int16_t *__restrict__ ref, uint32_t W, uint32_t nw, uint32_t *slot, uint32_t lane) {
        if (kb == KB) dirs_walk<G, KB, true>(L, ref, W, nw, slot, lane);
        else if constexpr (KB + 1 < G) WinWalk<G, KB + 1>::run(kb, L, ref, W, nw, slot, lane);
    }
};

template <int G>
__global__ __launch_bounds__(256) void k_sdtw_win(uint32_t n, WinArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;                                                // (the wave's branch: `read` is the same in its 64 lanes)
    const uint32_t Q = wave_rows(A.qlen[read], A.qpitch);
    if (other_launch<G>(Q)) return;
    int32_t st = A.gate ? A.gate[read] : 0;
    uint32_t W = 0, ws = 0;
    if (st == 0 && Q) st = win_row_check(A.rows_in[read], Q, A.R, A.pad, A.wmax, &ws, &W);
    st = (int32_t)sgpr((uint32_t)st);
    W = sgpr(W);
    ws = sgpr(ws);
    const bool path = Q != 0 && st == 0;
    int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
    for (uint32_t x = (path ? Q : 0u) + lane; x < A.qpitch; x += 64u) { lo[x] = -1; hi[x] = -1; }
    if (lane == 0) A.status[read] = st;
    if (!path) {                                                          // (wave-uniform)
        if (lane == 0) A.rows_out[read] = result_row(NO_COST, 0, -1, -1);
        return;
    }
    Lane<G, false> L;
    lane_init(L, lane == 0);
    const int16_t *q = A.queries + read * A.qpitch;
#pragma unroll
    for (int k = 0; k < G; k++) L.q[k] = query_value(q, lane * G + k, Q);
    const uint32_t last = (Q - 1) / G;                                     // the lane of row Q - 1 ...
    const int kb = (int)(Q - 1 - last * G);                                // ... and which of its rows it is
    const uint32_t nw = walk_words<G>(W, last, A.slot_words);
    uint32_t *slot = A.scratch + read * ((uint64_t)A.slot_words * 64u) + lane;
    WinWalk<G>::run(kb, L, A.ref + ws, W, nw, slot, lane);
    if (lane == last) A.rows_out[read] = result_row(L.best, Q, -1, (int32_t)ws + L.best_end);
}

__global__ __launch_bounds__(64) void k_sdtw_trace_win(uint32_t n, WinArgs A) {
    const uint64_t read = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (read >= n) return;
    const uint32_t Q = rows_of(A.qlen[read], A.qpitch);
    if (Q == 0 || (A.gate && A.gate[read] != 0)) return;
    uint32_t W, ws;
    if (win_row_check(A.rows_in[read], Q, A.R, A.pad, A.wmax, &ws, &W) != 0) return;   // (k_sdtw_win wrote the status, the empty row and the -1s)
    int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
    U4 row = A.rows_out[read];
    const uint32_t jend = row.w - ws;                                      // (end' < ws: far above W)
    int32_t rc = S5GPU_STATUS_PATH_ROW, start = -1;
    if (row.y == Q && jend < W)
        rc = path_walk_from(A.scratch + read * ((uint64_t)A.slot_words * 64u), A.slot_words, lane_height(Q), Q, W, (int32_t)ws, jend, lo, hi, &start);
    if (rc != 0) {
        for (uint32_t i = 0; i < Q; i++) { lo[i] = -1; hi[i] = -1; }
        A.status[read] = rc;
        A.rows_out[read] = result_row(NO_COST, 0, -1, -1);
        return;
    }
    row.z = (uint32_t)start;
    A.rows_out[read] = row;
}

// round 0: the outputs from what came in.  round k >= 1: where the trial round succeeded it becomes the read's result; where it did not the
// read keeps what it has and takes its status (a path that did not pass k_path_fit's checks: the read has no result at all).
__global__ __launch_bounds__(256) void k_refine_round(uint32_t n, RoundArgs A, uint32_t round) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;
    const uint32_t Q = wave_rows(A.qlen[read], A.qpitch);
    const uint64_t at = read * A.qpitch;
    int mode;                                                             // 0 nothing, 1 from what came in, 2 from the trial, 3 no result
    int32_t st = 0;
    if (round == 0) {
        st = __builtin_amdgcn_readfirstlane(A.status_in[read]);
        mode = st != 0 || Q == 0 ? 3 : 1;
    } else {
        const int32_t cur = __builtin_amdgcn_readfirstlane(A.status[read]);
        if (cur != 0 || Q == 0) return;                                   // (wave-uniform: the read takes no part any more)
        const int32_t sf = __builtin_amdgcn_readfirstlane(A.t_st_fit[read]), sw = __builtin_amdgcn_readfirstlane(A.t_st_win[read]);
        st = sf ? sf : sw;
        mode = st == 0 ? 2 : sf == S5GPU_STATUS_PATH_ROW || sf == S5GPU_STATUS_PATH_WIDE ? 3 : 0;
    }
    if (mode) {
        for (uint32_t x = lane; x < A.qpitch; x += 64u) {
            const bool in = x < Q;
            int16_t v = 0;
            int32_t l = -1, h = -1;
            if (mode == 1 && in) { v = A.q_in[at + x]; l = A.lo_in[at + x]; h = A.hi_in[at + x]; }
            if (mode == 2) { v = A.t_q[at + x]; l = A.t_lo[at + x]; h = A.t_hi[at + x]; }
            A.q[at + x] = v; A.lo[at + x] = l; A.hi[at + x] = h;
        }
    }
    if (lane == 0) {
        if (mode == 1) A.rows[read] = A.rows_in[read];
        if (mode == 2) { A.rows[read] = A.t_rows[read]; A.fit[read] = A.t_fit[read]; A.rounds[read] = round; }
        if (mode == 3) A.rows[read] = result_row(NO_COST, 0, -1, -1);
        if (mode == 1 || mode == 3) { A.fit[read] = fit_none(); A.rounds[read] = 0; }
        if (round == 0 || st != 0) A.status[read] = st;
    }
}

int refk::launch_fit(uint32_t n, const FitArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_path_fit, dim3((uint32_t)(((uint64_t)n + 3u) / 4u)), dim3(256), 0, st, n, A);
    S5_LAUNCH_CHECK("k_path_fit");
    return S5GPU_OK;
}

// a launch per lane height that a query of at most qpitch rows can need; then the trace
int refk::launch_window(uint32_t n, const WinArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    const int rc = for_each_lane_height(A.qpitch, [&](auto g) -> int {
        hipLaunchKernelGGL((k_sdtw_win<decltype(g)::value>), wave_grid(n), dim3(256), 0, st, n, A);
        S5_LAUNCH_CHECK("k_sdtw_win");
        return S5GPU_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_sdtw_trace_win, dim3((uint32_t)(((uint64_t)n + 63u) / 64u)), dim3(64), 0, st, n, A);
    S5_LAUNCH_CHECK("k_sdtw_trace_win");
    return S5GPU_OK;
}

int refk::launch_round(uint32_t n, const RoundArgs &A, uint32_t round, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_refine_round, dim3((uint32_t)(((uint64_t)n + 3u) / 4u)), dim3(256), 0, st, n, A, round);
    S5_LAUNCH_CHECK("k_refine_round");
    return S5GPU_OK;
}
