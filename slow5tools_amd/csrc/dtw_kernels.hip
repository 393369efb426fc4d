// dtw_kernels.hip — subsequence DTW of each read's events against a reference squiggle on the device (docs/codecs.md §4.16):
//   k_ev_query : per read, the quantised means of its event rows [skip, skip + qlen) as a row of the [n, qmax] int16 query matrix
//   k_sdtw     : per read, (cost, qlen, start, end) of the best alignment of its query to a piece of the reference
//   k_sdtw2    : k_sdtw, and (cost2, end2, mapq) of the best hit at least two blocks of columns away (§4.19), in the same pass
// k_sdtw is the project's one O(query x reference) kernel: a wave per read, systolic.  Lane l owns rows [l G, (l + 1) G) of the DTW matrix
// (G = 1, 2, 4, 8, 16: the smallest with 64 G >= qlen, a kernel each), its query values and its cells of the column it did last in
// registers.  At step t lane l does column t - l: from lane l - 1 it takes that lane's bottom cell of the same column (what it took one
// step earlier is the diagonal) and the reference value, one DPP wave shift each; lane 0 gets the reference value by v_readlane from a
// 64-value block that the wave loads together every 64 steps.  A cell is min3, absolute difference, add on uint32: D < 2^26 (§4.16).
// Every lane steps at every step, before its column 0 and behind column R - 1 too (dtw_dev.h, FAR): no step has a predicate.
// The pieces of the kernels' head, the walk over the steps and the launch per lane height are dtw_dev.h's (wave_read, wave_rows,
// other_launch, query_value; sdtw_walk; for_each_lane_height): the path kernels share them.  k_sdtw2 alone keeps its own head and walk.
// Nothing can index outside what it owns by construction (the rules of signal_kernels.hip):
//   1. trip counts come from R and qlen only (qlen clamped to the pitch and to 64 G);
//   2. no sample, cost or position forms an address: `end` and `start` are written as values;
//   3. a wave shares nothing but the shifts, which every lane executes: there is no barrier and no LDS;
//   4. a wave writes the one 16-byte row of its read; k_ev_query writes row i of the matrix, qlen[i] and status[i] of its read.
#include "dev_common.h"
#include "dtw_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace dtwk;

// a read per lane: at most qmax <= 1024 means each, a negligible share of the work
__global__ __launch_bounds__(256) void k_ev_query(uint32_t n, QueryArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t f0 = A.first[i], f1 = A.first[i + 1];
    const uint64_t E = f1 > f0 ? f1 - f0 : 0;
    const uint64_t avail = E > A.skip ? E - A.skip : 0;
    uint32_t ql = avail < A.qmax ? (uint32_t)avail : A.qmax;
    int32_t st = A.ev_status ? A.ev_status[i] : 0;
    if (st != 0) ql = 0;                                                  // the rows of a failed record or an overflowed slot are no query
    else if (ql < A.qmin) { ql = 0; st = S5GPU_STATUS_QUERY_SHORT; }
    int16_t *q = A.queries + i * A.qmax;
    if (ql) quant_row(&A.rows[f0 + A.skip].mean, sizeof(s5gpu_event_t) / sizeof(float), ql, A.scale, A.clip, q);
    for (uint32_t j = ql; j < A.qmax; j++) q[j] = 0;
    A.qlen[i] = ql;
    A.status[i] = st;
}

template <int G, bool WS>
__global__ __launch_bounds__(256) void k_sdtw(uint32_t n, const int16_t *__restrict__ queries, uint32_t qpitch, const uint32_t *__restrict__ qlen,
                                              const int16_t *__restrict__ ref, uint32_t R, U4 *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;                                                // (the wave's branch: `read` is the same in its 64 lanes)
    const uint32_t Q = wave_rows(qlen[read], qpitch);
    if (other_launch<G>(Q)) return;
    if (Q == 0) {
        if (lane == 0) out[read] = result_row(NO_COST, 0, -1, -1);
        return;
    }
    Lane<G, WS> L;
    lane_init(L, lane == 0);
    const int16_t *q = queries + read * qpitch;
#pragma unroll
    for (int k = 0; k < G; k++) L.q[k] = query_value(q, lane * G + k, Q);
    const uint32_t last = (Q - 1) / G;                                     // the lane of row Q - 1 ...
    const int kb = (int)(Q - 1 - last * G);                                // ... and which of its rows it is
    with_kb<G>(kb, [&](auto KB) { sdtw_walk<G, WS, decltype(KB)::value>(L, ref, R, last, lane); });
    if (lane == last) out[read] = result_row(L.best, Q, WS ? L.best_start : -1, L.best_end);
}

// ---- k_sdtw2: k_sdtw with the second-best hit (§4.19).  It keeps its kernel text, walk and dispatch to itself: on the shared ones
// (sdtw_walk behind `if constexpr`, with_kb) it measured 0.2 to 0.4 % behind, the loop laid out differently, the cause not found.
// The walk of sdtw_walk with lane_second beside lane_best, and second_flush where the
// lane of row Q - 1 has done the last column of a block: it does column t - last at step t, both the same in the whole wave, and a block is at
// least the 64 steps of a reference block long, so in every 64 steps there is at most one such step, kf, found once: a scalar compare and
// branch per step, taken once per block, every lane with it (the other lanes' lists are never read).
template <int G, bool WS, int KB>
__device__ __forceinline__ void sdtw_walk2(Lane<G, WS> &L, Second &S, const int16_t *__restrict__ ref, uint32_t R, uint32_t last, uint32_t lane,
                                           uint32_t bshift) {
    const uint32_t steps = R + last, mask = (1u << bshift) - 1u;
    uint32_t rcur = 0;
    uint32_t j = 0u - lane;
    auto step = [&](uint32_t rblk, uint32_t k, uint32_t t, uint32_t kf) {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)rblk, (int)k);
        rcur = shift_up1(rcur, r0);
        const uint32_t up = shift_up1_zero(L.d[G - 1]);
        const int32_t sup = WS ? (int32_t)shift_up1((uint32_t)L.s[G - 1], t + 1) : -1;
        lane_step(L, rcur, up, sup);
        lane_best<G, WS, KB>(L, j, R);
        lane_second<G, WS, KB>(L, S, j, R);
        if (k == kf) second_flush(S);
        j++;
    };
    constexpr int UNROLL = G >= 8 ? 2 : 8;
    uint32_t tb = 0;
    for (; tb + 64 <= steps; tb += 64) {
        const uint32_t at = tb + lane;
        const uint32_t rblk = biased(at < R ? ref[at] : (int16_t)0);
        const uint32_t kf = (last + mask - tb) & mask;                     // (tb + kf - last) & mask == mask; 64 or more: not in these steps
#pragma unroll UNROLL
        for (uint32_t k = 0; k < 64; k++) step(rblk, k, tb + k, kf);
    }
    if (tb < steps) {
        const uint32_t at = tb + lane;
        const uint32_t rblk = biased(at < R ? ref[at] : (int16_t)0);
        const uint32_t kf = (last + mask - tb) & mask;
        for (uint32_t k = 0; k < steps - tb; k++) step(rblk, k, tb + k, kf);
    }
    second_flush(S);                                                       // column R - 1 (nothing, where it ended a block)
}
template <int G, bool WS, int KB = 0>
struct Walk2 {
    static __device__ __forceinline__ void run(int kb, Lane<G, WS> &L, Second &S, const int16_t *__restrict__ ref, uint32_t R, uint32_t last,
                                               uint32_t lane, uint32_t bshift) {
        if (kb == KB) sdtw_walk2<G, WS, KB>(L, S, ref, R, last, lane, bshift);
        else if constexpr (KB + 1 < G) Walk2<G, WS, KB + 1>::run(kb, L, S, ref, R, last, lane, bshift);
    }
};

template <int G, bool WS>
__global__ __launch_bounds__(256) void k_sdtw2(uint32_t n, const int16_t *__restrict__ queries, uint32_t qpitch, const uint32_t *__restrict__ qlen,
                                               const int16_t *__restrict__ ref, uint32_t R, uint32_t bshift, U4 *__restrict__ out,
                                               U4 *__restrict__ out2) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (read >= n) return;
    uint32_t Q = qlen[read];
    Q = Q < qpitch ? Q : qpitch;
    Q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(Q < QMAX ? Q : QMAX));
    if (Q > 64u * G || (G > 1 && Q <= 32u * G)) return;                    // another launch's read
    Second S;
    second_init(S);
    if (Q == 0) {
        if (lane == 0) { out[read] = result_row(NO_COST, 0, -1, -1); out2[read] = second_row(S, bshift); }
        return;
    }
    Lane<G, WS> L;
    lane_init(L, lane == 0);
    const int16_t *q = queries + read * qpitch;
#pragma unroll
    for (int k = 0; k < G; k++) {
        const uint32_t row = lane * G + k;
        L.q[k] = biased(row < Q ? q[row] : (int16_t)0);
    }
    const uint32_t last = (Q - 1) / G;
    const int kb = (int)(Q - 1 - last * G);
    Walk2<G, WS>::run(kb, L, S, ref, R, last, lane, bshift);
    if (lane == last) { out[read] = result_row(L.best, Q, WS ? L.best_start : -1, L.best_end); out2[read] = second_row(S, bshift); }
}

int dtwk::launch_queries(uint32_t n, const QueryArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_ev_query, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, st, n, A);
    S5_LAUNCH_CHECK("k_ev_query");
    return S5GPU_OK;
}

int dtwk::launch_sdtw(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, bool want_start,
                      s5gpu_map_row_t *out, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    U4 *o = reinterpret_cast<U4 *>(out);
    return for_each_lane_height(qpitch, [&](auto g) -> int {
        constexpr int G = decltype(g)::value;
        if (want_start) hipLaunchKernelGGL((k_sdtw<G, true>), wave_grid(n), dim3(256), 0, st, n, queries, qpitch, qlen, ref, R, o);
        else hipLaunchKernelGGL((k_sdtw<G, false>), wave_grid(n), dim3(256), 0, st, n, queries, qpitch, qlen, ref, R, o);
        S5_LAUNCH_CHECK("k_sdtw");
        return S5GPU_OK;
    });
}

int dtwk::launch_sdtw2(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, bool want_start,
                       uint32_t bshift, s5gpu_map_row_t *out, s5gpu_map_second_t *out2, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    U4 *o = reinterpret_cast<U4 *>(out), *o2 = reinterpret_cast<U4 *>(out2);
    return for_each_lane_height(qpitch, [&](auto g) -> int {
        constexpr int G = decltype(g)::value;
        if (want_start) hipLaunchKernelGGL((k_sdtw2<G, true>), wave_grid(n), dim3(256), 0, st, n, queries, qpitch, qlen, ref, R, bshift, o, o2);
        else hipLaunchKernelGGL((k_sdtw2<G, false>), wave_grid(n), dim3(256), 0, st, n, queries, qpitch, qlen, ref, R, bshift, o, o2);
        S5_LAUNCH_CHECK("k_sdtw2");
        return S5GPU_OK;
    });
}
