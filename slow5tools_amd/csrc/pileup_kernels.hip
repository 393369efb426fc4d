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
// Whole reads (§4.22): the ragged layout of s5gpu_sdtw_band_dev, the unit of work a segment of S rows of one read.  The layout, the walks
// over the segments and rules 7 to 11 are in ragged_dev.h; beside them 2, 3 (per row), 5 and 6 hold here.
//   k_pileup_long_plan  : one workgroup: the layout checks of every read -> its verdict word; P, the exclusive prefix of the reads' segments
//   k_pileup_long_check : a wave per segment validates its rows (the first against the row before it in the ragged array); a failure ORs
//                         V_BAD into the read's verdict.  The kernel boundary makes the verdicts final.  With the sort on it also counts
//                         the segments by the column block of their first lo.
//   k_pileup_long_scan  : the rest of the counting sort: the counts' prefix, then k_pileup_long_check once more (pass 1) as the scatter
//                         that writes the segments (read, segment) in the order of that key
//   k_pileup_long_accum : k_pileup over a slice of the (ordered) segments, a wave per segment at a time; segments of reads whose verdict
//                         is not V_USED are passed over; the reads are counted once each, from the verdicts
// The level histograms of §4.23 (contrast_kernels.hip) and refine over whole reads (§4.24, refine_long_kernels.hip) run behind the same plan
// and check passes.
#include <string.h>

#include "dev_common.h"
#include "pileup_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

namespace {

uint32_t g_cols = MAX_COLS;        // option "pileup_lds_cols"
uint32_t g_grid = MAX_GRID;        // option "pileup_grid"
uint32_t g_long_seg = 256;         // option "pileup_long_seg"
uint32_t g_long_cols = MAX_COLS;   // option "pileup_long_cols"
uint32_t g_long_sort = 1;          // option "pileup_long_sort"
uint32_t g_long_grid = MAX_GRID;   // option "pileup_long_grid"
uint32_t g_long_passes = 7;        // option "pileup_long_passes"

// The LDS window of k_pileup and k_pileup_long_accum, cols columns of COL_WORDS words: emptied by the workgroup (a barrier follows at the
// caller), and behind the barrier that ends the adds its non-empty columns added to the table
__device__ __forceinline__ void win_clear(uint64_t *win, uint32_t cols) {
    for (uint32_t t = threadIdx.x; t < cols * COL_WORDS; t += s5::NT) win[t] = t % COL_WORDS == 5 ? EMPTY_MINMAX : 0ull;
}
__device__ __forceinline__ void win_flush(const Window &W, s5gpu_pile_col_t *win, s5gpu_pile_col_t *table, uint32_t R) {
    for (uint32_t b = threadIdx.x; b < W.cols; b += s5::NT) {
        const uint32_t j = W.lo + b;
        if (j >= W.lo && j < R) col_merge<DevOps>(table + j, win + b);
    }
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
    win_clear(pile_win, cols);
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
    win_flush(W, win, table, A.R);
    head_add(head, {used, skipped, bad, wave_sum(cells), wave_sum(cost)});
}

int pilek::set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    const bool pow2 = value > 0 && (value & (value - 1)) == 0;
    if (strcmp(key, "pileup_lds_cols") == 0 && (value == 0 || (pow2 && value >= (long)MIN_COLS && value <= (long)MAX_COLS))) {
        g_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pileup_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_grid = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "pileup_long_seg") == 0 && pow2 && value >= (long)SEG_MIN && value <= (long)SEG_MAX) { g_long_seg = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "pileup_long_cols") == 0 && (value == 0 || (pow2 && value >= (long)MIN_COLS && value <= (long)MAX_COLS))) {
        g_long_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pileup_long_sort") == 0 && (value == 0 || value == 1)) { g_long_sort = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "pileup_long_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_long_grid = (uint32_t)value; return S5GPU_OK; }
    // which kernels a ragged call launches: 1 the plan, 2 the check (and the sort), 4 the accumulate, over what an earlier call left in the
    // work area; 7 all (the default).  For tools/pileup_long_time.py: the passes are timed apart (as "sdtw_band_passes").
    if (strcmp(key, "pileup_long_passes") == 0 && value >= 1 && value <= 7) { g_long_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int pilek::launch_reset(void *acc, uint32_t R, hipStream_t st) {
    const uint64_t words = HEAD_WORDS + (uint64_t)COL_WORDS * R, blocks = (words + s5::NT - 1) / s5::NT;
    hipLaunchKernelGGL(k_pileup_reset, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(s5::NT), 0, st, reinterpret_cast<uint64_t *>(acc), R);
    S5_LAUNCH_CHECK("k_pileup_reset");
    return S5GPU_OK;
}

int pilek::launch_add_skipped(void *acc, uint32_t k, hipStream_t st) {
    if (k == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_pileup_add_skipped, dim3(1), dim3(64), 0, st, reinterpret_cast<uint64_t *>(acc), k);
    S5_LAUNCH_CHECK("k_pileup_add_skipped");
    return S5GPU_OK;
}

int pilek::launch_pileup(uint32_t n, const PileArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    const uint32_t cols = g_cols, quads = (uint32_t)(((uint64_t)n + 3u) / 4u);
    const uint32_t want = quads < g_grid ? quads : g_grid;                 // a slice: whole groups of four reads, the same for every workgroup
    const uint64_t per = (uint64_t)((quads + want - 1) / want) * 4u;
    const uint32_t grid = (uint32_t)(((uint64_t)n + per - 1) / per);
    hipLaunchKernelGGL(k_pileup, dim3(grid), dim3(s5::NT), (size_t)cols * sizeof(s5gpu_pile_col_t), st, n, per, A, cols);
    S5_LAUNCH_CHECK("k_pileup");
    return S5GPU_OK;
}

// ---------------------------------------------------------------------------------------------------------------- whole reads (§4.22)

// One workgroup.  verdict[k] and P for every read; the sort's counts zeroed.
__global__ __launch_bounds__(s5::NT) void k_pileup_long_plan(PileLongArgs A, uint32_t S, LongPtrs L) {
    __shared__ uint32_t s_scan[s5::NT];
    __shared__ uint64_t s_carry;
    for (uint32_t t = threadIdx.x; t < LONG_KEYS; t += s5::NT) L.hist[t] = 0u;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint64_t c = 0; c < A.n; c += s5::NT) {                           // (the same trips for every thread)
        const uint64_t k = c + threadIdx.x;
        uint32_t segs = 0;
        if (k < A.n) {
            const uint32_t Q = A.qlen[k];
            const uint32_t v = long_verdict(A.first[k], A.first[k + 1], Q, A.status[k], A.total_rows, A.ev_skip);
            L.verdict[k] = v;
            segs = v == V_USED ? segs_of(Q, S) : 0u;
        }
        s_scan[threadIdx.x] = segs;
        __syncthreads();
        for (uint32_t d = 1; d < (uint32_t)s5::NT; d <<= 1) {               // inclusive, Hillis and Steele: at most 256 * 2^14
            const uint32_t add = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0u;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        const uint64_t carry = s_carry;
        if (k < A.n) L.P[k] = carry + s_scan[threadIdx.x] - segs;
        __syncthreads();
        if (threadIdx.x == s5::NT - 1) s_carry = carry + s_scan[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) L.P[A.n] = s_carry;
}

// A wave per segment, each wave a slice of the segments in P's order.  pass 0: the rows validated, and (sort) the segment counted under its
// key; pass 1 (sort only, behind k_pileup_long_scan): the segment put at its place in the ordered list.
__global__ __launch_bounds__(s5::NT) void k_pileup_long_check(PileLongArgs A, uint32_t S, LongPtrs L, uint32_t sort, uint32_t pass) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool sorted = sort && L.P[A.n] <= L.cap;
    if (pass == 1 && !sorted) return;                                      // (no barrier in this kernel)
    walk_by_wave(A, S, L, [&](const Seg &g) {
        const uint64_t f = A.first[g.k];
        const int32_t *lo = A.lo + f, *hi = A.hi + f;
        if (pass == 0) {
            const bool ok = seg_rows_ok(g.r0, g.r1, lane, 64u, lo, hi, A.R);
            if (!__all(ok ? 1 : 0) && lane == 0) atomicOr(&L.verdict[g.k], V_BAD);
        }
        if (sorted && lane == 0) {
            const uint32_t key = seg_key(lo[g.r0], A.R);
            if (pass == 0) atomicAdd(&L.hist[key], 1u);
            else {
                const uint64_t at = atomicAdd(&L.cursor[key], 1u);
                if (at < L.cap) L.order[at] = (uint64_t)g.k << 32 | g.s;
            }
        }
    });
}

// One workgroup of LONG_KEYS threads: cursor = the exclusive prefix of hist (32-bit counts: launch_pileup_long sorts below 2^32 segments only);
// hist is left zeroed, as the plan leaves it: a check pass launched again on its own (pileup_long_passes) counts from nothing
__global__ __launch_bounds__(LONG_KEYS) void k_pileup_long_scan(LongPtrs L) {
    __shared__ uint32_t s_scan[LONG_KEYS];
    const uint32_t own = L.hist[threadIdx.x];
    L.hist[threadIdx.x] = 0u;
    s_scan[threadIdx.x] = own;
    __syncthreads();
    for (uint32_t d = 1; d < LONG_KEYS; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0u;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    L.cursor[threadIdx.x] = s_scan[threadIdx.x] - own;
}

// per workgroup a slice of the (ordered) segments, a wave per segment at a time; cols as in k_pileup
__global__ __launch_bounds__(s5::NT) void k_pileup_long_accum(PileLongArgs A, uint32_t S, LongPtrs L, uint32_t sort, uint32_t cols) {
    extern __shared__ __attribute__((aligned(16))) uint64_t pile_win[];   // cols columns of COL_WORDS words
    __shared__ uint32_t s_lo;
    const uint32_t lane = threadIdx.x & 63u;
    win_clear(pile_win, cols);
    if (threadIdx.x == 0) s_lo = ANCHOR_NONE;
    __syncthreads();
    const GroupSlice G = group_slice(A, L, sort);
    const uint32_t wave = wave_of_group(), l0 = cols ? group_anchor(A, S, L, G, wave, wave + 1u) : ANCHOR_NONE;
    if (lane == 0 && l0 != ANCHOR_NONE) atomicMin(&s_lo, l0);
    __syncthreads();
    Window W;
    W.lo = s_lo == ANCHOR_NONE ? 0u : s_lo;
    W.cols = cols;
    s5gpu_pile_col_t *win = reinterpret_cast<s5gpu_pile_col_t *>(pile_win);
    uint64_t *head = reinterpret_cast<uint64_t *>(A.acc);
    s5gpu_pile_col_t *table = reinterpret_cast<s5gpu_pile_col_t *>(head + HEAD_WORDS);
    uint64_t cells = 0, cost = 0;                                          // this lane's
    walk_by_group(A, S, L, G, [&](const Seg &g) {
        const uint64_t f = A.first[g.k];                                   // (loaded beside the verdict: rule 7, k < n)
        if (L.verdict[g.k] != V_USED) return;                              // (the wave's branch)
        seg_cells<DevOps>(g.r0, g.r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, A.events ? A.events + f + A.ev_skip : nullptr, A.ref, A.R, W, win, table,
                          &cells, &cost);
    });
    __syncthreads();
    win_flush(W, win, table, A.R);
    const ReadCounts c = verdict_counts(L.verdict, A.n);
    head_add(head, {c.used, c.skipped, c.bad, wave_sum(cells), wave_sum(cost)});
}

uint32_t pilek::long_seg() { return g_long_seg; }

uint32_t pilek::long_grid(const PileLongArgs &A, uint32_t S, uint32_t most) {
    const uint64_t segs = A.total_rows / S + A.n, quads = (segs + 3u) / 4u;  // the segments of a well-formed layout, at most
    return (uint32_t)(quads < most ? quads : most);
}
uint32_t pilek::long_grid(const PileLongArgs &A, uint32_t S) { return long_grid(A, S, g_long_grid); }

int pilek::launch_long_plan_check(const PileLongArgs &A, hipStream_t st) {
    if (A.n == 0) return S5GPU_OK;
    const uint32_t S = g_long_seg;
    const LongPtrs L = long_ptrs(A);
    hipLaunchKernelGGL(k_pileup_long_plan, dim3(1), dim3(s5::NT), 0, st, A, S, L);
    S5_LAUNCH_CHECK("k_pileup_long_plan");
    hipLaunchKernelGGL(k_pileup_long_check, dim3(long_grid(A, S)), dim3(s5::NT), 0, st, A, S, L, 0u, 0u);
    S5_LAUNCH_CHECK("k_pileup_long_check");
    return S5GPU_OK;
}

int pilek::launch_pileup_long(const PileLongArgs &A, hipStream_t st) { return launch_pileup_long(A, nullptr, st); }

int pilek::launch_pileup_long(const PileLongArgs &A, void *hist, hipStream_t st) {
    if (A.n == 0) return S5GPU_OK;
    const uint32_t S = g_long_seg, cols = g_long_cols;
    const LongPtrs L = long_ptrs(A);
    // (the sort's counts are 32-bit: a list that 2^32 segments might not fit is walked in P's order)
    const uint32_t sort = g_long_sort && L.cap < ((uint64_t)1 << 32) ? 1u : 0u;
    const uint32_t grid = long_grid(A, S);
    const uint32_t passes = g_long_passes;
    if (passes & 1u) {
        hipLaunchKernelGGL(k_pileup_long_plan, dim3(1), dim3(s5::NT), 0, st, A, S, L);
        S5_LAUNCH_CHECK("k_pileup_long_plan");
    }
    if (passes & 2u) {
        hipLaunchKernelGGL(k_pileup_long_check, dim3(grid), dim3(s5::NT), 0, st, A, S, L, sort, 0u);
        S5_LAUNCH_CHECK("k_pileup_long_check");
    }
    if (sort && (passes & 2u)) {
        hipLaunchKernelGGL(k_pileup_long_scan, dim3(1), dim3(LONG_KEYS), 0, st, L);
        S5_LAUNCH_CHECK("k_pileup_long_scan");
        hipLaunchKernelGGL(k_pileup_long_check, dim3(grid), dim3(s5::NT), 0, st, A, S, L, sort, 1u);
        S5_LAUNCH_CHECK("k_pileup_long_check (scatter)");
    }
    if ((passes & 4u) && A.acc) {
        hipLaunchKernelGGL(k_pileup_long_accum, dim3(grid), dim3(s5::NT), (size_t)cols * sizeof(s5gpu_pile_col_t), st, A, S, L, sort, cols);
        S5_LAUNCH_CHECK("k_pileup_long_accum");
    }
    if ((passes & 4u) && hist) return launch_hist_accum(A, S, L, sort, hist, st);
    return S5GPU_OK;
}
