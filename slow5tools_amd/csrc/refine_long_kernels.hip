// refine_long_kernels.hip — refine over whole reads (docs/codecs.md §4.24): the fit of §4.20 along the ragged paths, behind the plan and the
// check of pileup_kernels.hip (no sort: there is no window to keep warm, the segments are walked in P's order, a wave's own run of them:
// walk_by_wave of ragged_dev.h), and the bookkeeping of the rounds of s5gpu_extend_refine_dev (refine_long_api.hip):
//   k_path_fit_long    : a wave per segment, each wave a slice of consecutive segments, lanes over rows.  A lane keeps its six partial sums
//                        while the wave stays in one read; where the read changes (and at the end) the wave reduces them with shuffles and
//                        lane 0 adds them to the read's Sums with 64-bit atomics: integers, so the bytes depend on nothing but the cells
//   k_fit_long_solve   : a lane per read: verdict and sums -> fit and status (refk::long_fit_status)
//   k_requant_long     : over the same segments: q' = requant_one(q0) for the rows of the reads whose fit's status is 0
//   k_refine_long_gate : a lane per read: the status of a result row as a word of its own (what the plan and the band call read)
//   k_refine_long_round: over the same segments the rows of q, lo and hi a read takes over (refk::long_round_rule), and a lane per read its
//                        row, fit, rounds and status.  The statuses are read from one array and written to another: no wave reads what
//                        another writes.
// Rules 2, 3 (per row) and 6 of pileup_kernels.hip and 7 to 9 and 11 of ragged_dev.h hold as they stand: nothing of a read is summed,
// requantised or copied unless its verdict is V_USED behind the check pass (in round 0 that of the path that came in), so first[k] + i lies
// inside the ragged arrays for i < Q; ref[j] is read behind j < R (row_sums); a[], b[] and the statuses are read at [read] for read < n.
// No barrier, no LDS; branches on a read's fate are wave-uniform, and every shuffle is executed by all 64 lanes.
#include <string.h>

#include "dev_common.h"
#include "pileup_dev.h"
#include "refine_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

namespace {
uint32_t g_refine_passes = 63;          // option "refine_long_passes"

__device__ __forceinline__ int64_t wave_sum_i(int64_t v) { return (int64_t)wave_sum((uint64_t)v); }
// the wave's partial sums of read `k` added to its Sums, and emptied (k = n: no read yet)
__device__ __forceinline__ void fit_flush(refk::Sums *sums, uint32_t k, uint32_t n, refk::Sums &acc, uint32_t lane) {
    if (k >= n) return;                                                    // (wave-uniform)
    const int64_t cnt = wave_sum_i(acc.n), sq = wave_sum_i(acc.sq), sr = wave_sum_i(acc.sr), sqq = wave_sum_i(acc.sqq), sqr = wave_sum_i(acc.sqr),
                  srr = wave_sum_i(acc.srr);
    if (lane == 0 && cnt != 0) {
        uint64_t *w = reinterpret_cast<uint64_t *>(sums + k);
        DevOps::add64(w + 0, (uint64_t)cnt); DevOps::add64(w + 1, (uint64_t)sq); DevOps::add64(w + 2, (uint64_t)sr);
        DevOps::add64(w + 3, (uint64_t)sqq); DevOps::add64(w + 4, (uint64_t)sqr); DevOps::add64(w + 5, (uint64_t)srr);
    }
    acc.n = acc.sq = acc.sr = acc.sqq = acc.sqr = acc.srr = 0;
}
}  // namespace

__global__ __launch_bounds__(s5::NT) void k_path_fit_long(PileLongArgs A, uint32_t S, LongPtrs L, refk::Sums *sums) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t held = A.n;
    refk::Sums acc = {0, 0, 0, 0, 0, 0};
    walk_by_wave(A, S, L, [&](const Seg &g) {
        if (L.verdict[g.k] != V_USED) return;                              // (the wave's branch)
        if (g.k != held) { fit_flush(sums, held, A.n, acc, lane); held = g.k; }
        const uint64_t f = A.first[g.k];
        refk::seg_sums(g.r0, g.r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, A.ref, A.R, acc);
    });
    fit_flush(sums, held, A.n, acc, lane);
}

__global__ __launch_bounds__(s5::NT) void k_fit_long_solve(uint32_t n, const uint32_t *__restrict__ verdict, const refk::Sums *__restrict__ sums,
                                                           const int32_t *__restrict__ status_in, s5gpu_refine_params_t P, s5gpu_fit_t *__restrict__ fit,
                                                           int32_t *__restrict__ status_out) {
    const uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x;
    if (k < n) {
        s5gpu_fit_t F;
        const int32_t st = refk::long_fit_status(verdict[k], status_in[k], sums[k], P, &F);
        fit[k] = F;
        status_out[k] = st;
    }
}

__global__ __launch_bounds__(s5::NT) void k_requant_long(PileLongArgs A, uint32_t S, LongPtrs L, const int32_t *__restrict__ fit_status,
                                                         const s5gpu_fit_t *__restrict__ fit, int32_t clip, int16_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    walk_by_wave(A, S, L, [&](const Seg &g) {
        if (L.verdict[g.k] != V_USED || fit_status[g.k] != 0) return;      // (the wave's branch)
        const uint64_t f = A.first[g.k];
        const double a = fit[g.k].a, b = fit[g.k].b;
        for (uint32_t i = g.r0 + lane; i < g.r1; i += 64u) out[f + i] = refk::requant_one(A.queries[f + i], a, b, clip);
    });
}

__global__ __launch_bounds__(s5::NT) void k_refine_long_gate(uint32_t n, const s5gpu_ext_row_t *__restrict__ rows, int32_t *__restrict__ st) {
    const uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x;
    if (k < n) st[k] = rows[k].status;
}

__global__ __launch_bounds__(s5::NT) void k_refine_long_round(refk::RoundLongArgs B, uint32_t round, uint32_t S, LongPtrs L) {
    const PileLongArgs &A = B.A;
    const uint32_t lane = threadIdx.x & 63u;
    walk_by_wave(A, S, L, [&](const Seg &g) {
        const uint32_t k = g.k, v = L.verdict[k];                          // (the wave's branches, as those below)
        if ((v & V_SKIPPED) || (round == 0 && v != V_USED)) return;        // (a bad path that came in: the fills hold "no result" already)
        int32_t st;
        const int mode = refk::long_round_rule(round, v, A.qlen[k], B.cur_in[k], round ? B.t_sf[k] : 0, round ? B.t_rows[k].status : 0, &st);
        if (mode == 0) return;
        const uint64_t f = A.first[k];                                     // (the read has segments: its layout passed this round's plan)
        for (uint32_t i = g.r0 + lane; i < g.r1; i += 64u) {
            int16_t q = 0;
            int32_t l = -1, h = -1;
            if (mode == 1) { q = A.queries[f + i]; l = A.lo[f + i]; h = A.hi[f + i]; }
            if (mode == 2) { q = B.t_q[f + i]; l = B.t_lo[f + i]; h = B.t_hi[f + i]; }
            B.q[f + i] = q; B.lo[f + i] = l; B.hi[f + i] = h;
        }
    });
    // the reads, once each
    for (uint64_t r = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; r < A.n; r += (uint64_t)gridDim.x * s5::NT) {
        int32_t st;
        const int mode = refk::long_round_rule(round, L.verdict[r], A.qlen[r], B.cur_in[r], round ? B.t_sf[r] : 0, round ? B.t_rows[r].status : 0, &st);
        if (round == 0 || B.cur_in[r] == 0) B.rows[r] = refk::long_round_row(mode, st, round ? B.t_rows[r] : B.rows_in[r], B.rows[r]);
        if (mode == 2) { B.fit[r] = B.t_fit[r]; B.rounds[r] = round; }
        if (mode == 1 || mode == 3) { B.fit[r] = refk::fit_none(); B.rounds[r] = 0; }
        B.cur_out[r] = st;
    }
}

// which kernels the whole-read fit and its rounds launch: 1 the plan and the check, 2 the sums, 4 the solve, 8 the requantiser, 16 the
// bookkeeping of the rounds, 32 the band call, over what an earlier call left; 63 all (the default).  For tools/extend_refine_time.py: the
// passes are timed apart.
int refk::long_set_option(const char *key, long value) {
    if (key && strcmp(key, "refine_long_passes") == 0 && value >= 1 && value <= 63) { g_refine_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

uint32_t refk::long_passes() { return g_refine_passes; }

int refk::launch_long_verdicts(const PileLongArgs &A, hipStream_t st) {
    if (!(g_refine_passes & 1u)) return S5GPU_OK;
    return launch_long_plan_check(A, st);
}

int refk::launch_fit_long(const FitLongArgs &F, hipStream_t st) {
    const PileLongArgs &A = F.A;
    if (A.n == 0) return S5GPU_OK;
    int rc;
    if ((rc = launch_long_verdicts(A, st))) return rc;
    const uint32_t S = long_seg(), grid = long_grid(A, S), per_read = (uint32_t)(((uint64_t)A.n + s5::NT - 1) / s5::NT);
    const LongPtrs L = long_ptrs(A);
    refk::Sums *sums = (refk::Sums *)((uint8_t *)A.work + fit_long_work(A.n, A.total_rows).o_sums);
    if (g_refine_passes & 2u) {
        const hipError_t e = hipMemsetAsync(sums, 0, sizeof(refk::Sums) * (size_t)A.n, st);
        if (e != hipSuccess) { s5gpu_set_error("k_path_fit_long: the sums could not be cleared: %s", hipGetErrorString(e)); return S5GPU_ERR_HIP; }
        hipLaunchKernelGGL(k_path_fit_long, dim3(grid), dim3(s5::NT), 0, st, A, S, L, sums);
        S5_LAUNCH_CHECK("k_path_fit_long");
    }
    if (g_refine_passes & 4u) {
        hipLaunchKernelGGL(k_fit_long_solve, dim3(per_read), dim3(s5::NT), 0, st, A.n, L.verdict, sums, A.status, F.P, F.fit, F.status_out);
        S5_LAUNCH_CHECK("k_fit_long_solve");
    }
    if (F.queries_out && (g_refine_passes & 8u)) {
        hipLaunchKernelGGL(k_requant_long, dim3(grid), dim3(s5::NT), 0, st, A, S, L, F.status_out, F.fit, F.P.clip, F.queries_out);
        S5_LAUNCH_CHECK("k_requant_long");
    }
    return S5GPU_OK;
}

int refk::launch_gate_long(uint32_t n, const s5gpu_ext_row_t *rows, int32_t *st_out, hipStream_t st) {
    if (n == 0 || !(g_refine_passes & 16u)) return S5GPU_OK;
    hipLaunchKernelGGL(k_refine_long_gate, dim3((uint32_t)(((uint64_t)n + s5::NT - 1) / s5::NT)), dim3(s5::NT), 0, st, n, rows, st_out);
    S5_LAUNCH_CHECK("k_refine_long_gate");
    return S5GPU_OK;
}

int refk::launch_round_long(const RoundLongArgs &B, uint32_t round, hipStream_t st) {
    if (B.A.n == 0 || !(g_refine_passes & 16u)) return S5GPU_OK;
    const uint32_t S = long_seg();
    hipLaunchKernelGGL(k_refine_long_round, dim3(long_grid(B.A, S)), dim3(s5::NT), 0, st, B, round, S, long_ptrs(B.A));
    S5_LAUNCH_CHECK("k_refine_long_round");
    return S5GPU_OK;
}
