// pileup_kernels.hip — per-reference-position statistics of aligned events (docs/codecs.md §4.18): one table of R columns stays on the
// device and k_pileup adds the cells of every used read of a batch to it.  Every member is an integer sum, min or max, so the result does
// not depend on the launch shape, on where a workgroup's window lies or on the order of the adds.
//   k_pileup_reset : the empty accumulator: zeros, the 32767 / -32768 pairs and R
//   k_pileup       : a workgroup of four waves walks a slice of consecutive reads, a wave per read at a time, lanes over the rows
//                    i = lane, lane + 64, ...  The wave validates the WHOLE read (one vote, a wave-uniform branch), then counts it and
//                    adds its cells.  The workgroup keeps a window of columns in LDS, anchored at the smallest lo[0] of the first reads it
//                    meets: cells inside go to LDS (64-bit adds, 32-bit min / max), the others straight to the table with global atomics;
//                    the non-empty columns of the window are added to the table at the workgroup's end.
// Values read from memory form addresses here (lo, hi).  The rules, those of dtw_path_kernels.hip:
//   1. nothing is accumulated before every row of the read has passed pilek::row_ok: 0 <= lo <= hi < R, lo[i] - hi[i - 1] in {0, 1};
//   2. a table column is cols[j] behind j < R (checked again in row_cells); a window slot is masked behind its range test (window_slot);
//   3. a row's loop has hi - lo + 1 <= R trips, a read at most Q + R cells; Q is qlen clamped to the pitch and to 1024;
//   4. queries, lo, hi and events are read at [read * qpitch + row] for row < Q only, qlen and status at [read] for read < n;
//   5. the only barriers are those around the LDS reset and the flush, reached by every thread: no thread returns early;
//   6. vector stores and HIP atomics only, no inline assembly.
#include <string.h>

#include "dev_common.h"
#include "pileup_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

namespace {

uint32_t g_cols = MAX_COLS;        // option "pileup_lds_cols"
uint32_t g_grid = MAX_GRID;        // option "pileup_grid"

struct DevOps {
    static __device__ __forceinline__ void add64(uint64_t *p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }
    // min_q and max_q only ever move one way, so a value read before (however stale) can only ask for an atomic too many, never one too few:
    // most cells of a column that holds a few reads already change neither
    static __device__ __forceinline__ void minmax32(s5gpu_pile_col_t *c, int32_t lo, int32_t hi) {
        const uint64_t mm = __hip_atomic_load(reinterpret_cast<uint64_t *>(&c->min_q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lo < (int32_t)(uint32_t)mm) atomicMin(&c->min_q, lo);
        if (hi > (int32_t)(uint32_t)(mm >> 32)) atomicMax(&c->max_q, hi);
    }
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

}  // namespace

__global__ __launch_bounds__(s5::NT) void k_pileup_reset(uint64_t *__restrict__ w, uint32_t R) {
    const uint64_t words = HEAD_WORDS + (uint64_t)COL_WORDS * R;
    for (uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; k < words; k += (uint64_t)gridDim.x * s5::NT) {
        uint64_t v = 0;
        if (k == 5) v = R;                                                // s5gpu_pile_total_t::R, the reserved words 0
        if (k >= HEAD_WORDS && (k - HEAD_WORDS) % COL_WORDS == 5) v = EMPTY_MINMAX;
        w[k] = v;
    }
}

__global__ void k_pileup_add_skipped(uint64_t *acc, uint32_t k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) DevOps::add64(acc + 1, k);
}

// per: the reads of a workgroup's slice, a multiple of 4; cols: the window's columns, 0 or a power of two (cols * 48 bytes of dynamic LDS)
__global__ __launch_bounds__(s5::NT) void k_pileup(uint32_t n, uint64_t per, PileArgs A, uint32_t cols) {
    extern __shared__ __attribute__((aligned(16))) uint64_t pile_win[];   // cols columns of COL_WORDS words
    __shared__ uint32_t s_lo;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t t = threadIdx.x; t < cols * COL_WORDS; t += s5::NT) pile_win[t] = t % COL_WORDS == 5 ? EMPTY_MINMAX : 0ull;
    if (threadIdx.x == 0) s_lo = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t base = blockIdx.x * per;
    const uint64_t end = base + per < n ? base + per : n;
    // the anchor: the smallest lo[0] of the reads the four waves meet first (where it lies changes the time, never the result)
    if (cols && lane == 0 && base + wave < end) {
        const uint64_t r0 = base + wave;
        if (A.status[r0] == 0 && rows_of(A.qlen[r0], A.qpitch) != 0) {
            const int32_t l0 = A.lo[r0 * A.qpitch];
            if (l0 >= 0 && (uint32_t)l0 < A.R) atomicMin(&s_lo, (uint32_t)l0);
        }
    }
    __syncthreads();
    Window W;
    W.lo = s_lo == 0xFFFFFFFFu ? 0u : s_lo;
    W.cols = cols;
    s5gpu_pile_col_t *win = reinterpret_cast<s5gpu_pile_col_t *>(pile_win);
    uint64_t *head = reinterpret_cast<uint64_t *>(A.acc);
    s5gpu_pile_col_t *table = reinterpret_cast<s5gpu_pile_col_t *>(head + HEAD_WORDS);

    uint64_t used = 0, skipped = 0, bad = 0;                               // the same in every lane of the wave
    uint64_t cells = 0, cost = 0;                                          // this lane's
    for (uint64_t read = base + wave; read < end; read += 4u) {
        const uint32_t Q = (uint32_t)__builtin_amdgcn_readfirstlane((int)rows_of(A.qlen[read], A.qpitch));
        const int32_t st = __builtin_amdgcn_readfirstlane(A.status[read]);
        if (st != 0 || Q == 0) { skipped++; continue; }                    // (the wave's branch)
        const int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
        bool ok = true;
        for (uint32_t i = lane; i < Q; i += 64u) ok = ok && row_ok(i, lo[i], hi[i], i ? hi[i - 1] : 0, A.R);
        if (!__all(ok ? 1 : 0)) { bad++; continue; }                       // one vote: the whole read or nothing of it
        used++;
        const int16_t *q = A.queries + read * A.qpitch;
        const s5gpu_event_t *ev = A.events ? A.events + read * A.qpitch : nullptr;
        for (uint32_t i = lane; i < Q; i += 64u)
            row_cells<DevOps>(i, lo[i], hi[i], i ? hi[i - 1] : 0, (int32_t)q[i], ev ? ev[i].length : 0u, A.ref, A.R, W, win, table, &cells, &cost);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < cols; b += s5::NT) {               // the flush: the non-empty columns of the window
        const uint32_t j = W.lo + b;
        if (j >= W.lo && j < A.R) col_merge<DevOps>(table + j, win + b);
    }
    cells = wave_sum(cells);
    cost = wave_sum(cost);
    if (lane == 0) {
        if (used) DevOps::add64(head + 0, used);
        if (skipped) DevOps::add64(head + 1, skipped);
        if (bad) DevOps::add64(head + 2, bad);
        if (cells) DevOps::add64(head + 3, cells);
        if (cost) DevOps::add64(head + 4, cost);
    }
}

#define PILE_LAUNCH_CHECK(what)                                                           \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess) {                                                           \
            s5gpu_set_error("%s launch failed: %s", what, hipGetErrorString(e_));         \
            return S5GPU_ERR_HIP;                                                         \
        }                                                                                 \
    } while (0)

int pilek::set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    if (strcmp(key, "pileup_lds_cols") == 0 && (value == 0 || (value >= (long)MIN_COLS && value <= (long)MAX_COLS && (value & (value - 1)) == 0))) {
        g_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pileup_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_grid = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int pilek::launch_reset(void *acc, uint32_t R, hipStream_t st) {
    const uint64_t words = HEAD_WORDS + (uint64_t)COL_WORDS * R, blocks = (words + s5::NT - 1) / s5::NT;
    hipLaunchKernelGGL(k_pileup_reset, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(s5::NT), 0, st, reinterpret_cast<uint64_t *>(acc), R);
    PILE_LAUNCH_CHECK("k_pileup_reset");
    return S5GPU_OK;
}

int pilek::launch_add_skipped(void *acc, uint32_t k, hipStream_t st) {
    if (k == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_pileup_add_skipped, dim3(1), dim3(64), 0, st, reinterpret_cast<uint64_t *>(acc), k);
    PILE_LAUNCH_CHECK("k_pileup_add_skipped");
    return S5GPU_OK;
}

int pilek::launch_pileup(uint32_t n, const PileArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    const uint32_t cols = g_cols, quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    const uint32_t want = quads < g_grid ? quads : g_grid;                 // a slice: whole groups of four reads, the same for every workgroup
    const uint64_t per = (uint64_t)((quads + want - 1) / want) * 4u;
    const uint32_t grid = (uint32_t)(((uint64_t)n + per - 1) / per);
    hipLaunchKernelGGL(k_pileup, dim3(grid), dim3(s5::NT), (size_t)cols * sizeof(s5gpu_pile_col_t), st, n, per, A, cols);
    PILE_LAUNCH_CHECK("k_pileup");
    return S5GPU_OK;
}
