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
// Whole reads (§4.22): the ragged layout of s5gpu_sdtw_band_dev, the unit of work a segment of S rows of one read.
//   k_pileup_long_plan  : one workgroup: the layout checks of every read -> its verdict word; P, the exclusive prefix of the reads' segments
//   k_pileup_long_check : a wave per segment validates its rows (the first against the row before it in the ragged array); a failure ORs
//                         V_BAD into the read's verdict.  The kernel boundary makes the verdicts final.  With the sort on it also counts
//                         the segments by the column block of their first lo.
//   k_pileup_long_scan  : the rest of the counting sort: the counts' prefix, then k_pileup_long_check once more (pass 1) as the scatter
//                         that writes the segments (read, segment) in the order of that key
//   k_pileup_long_accum : k_pileup over a slice of the (ordered) segments, a wave per segment at a time; segments of reads whose verdict
//                         is not V_USED are passed over; the reads are counted once each, from the verdicts
//   k_pile_hist_accum   : the same walk into the level histograms of §4.23 (further down, with its own note)
//   k_path_fit_long, k_fit_long_solve, k_requant_long, k_refine_long_gate, k_refine_long_round : refine over whole reads (§4.24), behind
//                         the same plan and check passes (further down, with their own note)
// Their rules, beside 2, 3 (per row), 5 and 6 above:
//   7. first, qlen and status are read at [read] (first also at [read + 1]) for read < n; a read has segments only behind long_verdict:
//      first[k] + Q + ev_skip <= first[k + 1] <= total_rows, Q <= 2^20, so queries, lo, hi at [first[k] + i] and events at
//      [first[k] + ev_skip + i] are inside their arrays for every i < Q, and hi[first[k] + i - 1] for 0 < i;
//   8. trip counts come from qlen, R, S, n and total_rows: a segment has at most S rows, segment numbers run below P[n], the sum of
//      ceil(Q / S), and a step from one segment's read to the next's takes at most n trips in all;
//   9. nothing of a read is accumulated unless k_pileup_long_check has passed every row of every one of its segments;
//  10. the sort's key is clamped below LONG_KEYS and indexes the counts only; a position in the ordered list is used behind `< cap`, and
//      a list that would not fit (P[n] > cap: only a layout whose reads overlap) is not made: the segments are then walked in P's order;
//  11. branches on a read's or a segment's fate are wave-uniform: they depend on values every lane of the wave reads from the same address.
#include <string.h>

#include "dev_common.h"
#include "pileup_dev.h"
#include "refine_dev.h"

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
int set_option_long(const char *key, long value);

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

int pilek::set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    if (strcmp(key, "pileup_lds_cols") == 0 && (value == 0 || (value >= (long)MIN_COLS && value <= (long)MAX_COLS && (value & (value - 1)) == 0))) {
        g_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pileup_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_grid = (uint32_t)value; return S5GPU_OK; }
    return set_option_long(key, value);
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

namespace {

struct LongPtrs {
    uint32_t *verdict;               // [n]
    uint64_t *P;                     // [n + 1]
    uint32_t *hist, *cursor;         // [LONG_KEYS] each
    uint64_t *order;                 // [cap]: read << 32 | segment
    uint64_t cap;
};

// the slice [*b, *e) of `total` items that part `who` of `parts` takes
__device__ __forceinline__ void slice_of(uint64_t total, uint64_t who, uint64_t parts, uint64_t *b, uint64_t *e) {
    const uint64_t per = (total + parts - 1u) / parts;
    *b = who * per < total ? who * per : total;
    *e = *b + per < total ? *b + per : total;
}

}  // namespace

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
    const uint64_t total = L.P[A.n];
    const bool sorted = sort && total <= L.cap;
    if (pass == 1 && !sorted) return;                                      // (no barrier in this kernel)
    uint64_t g, end;
    slice_of(total, (uint64_t)blockIdx.x * s5::NW + (threadIdx.x >> 6), (uint64_t)gridDim.x * s5::NW, &g, &end);
    uint32_t k = g < end ? seg_find(L.P, A.n, g) : 0u;
    for (; g < end; g++) {
        k = seg_next(L.P, A.n, k, g);
        const uint32_t Q = A.qlen[k], s = (uint32_t)(g - L.P[k]);
        if (s >= segs_of(Q < LONG_QMAX ? Q : LONG_QMAX, S)) continue;      // (cannot be: P was made of these)
        uint32_t r0, r1;
        seg_rows(Q, S, s, &r0, &r1);
        const uint64_t f = A.first[k];
        const int32_t *lo = A.lo + f, *hi = A.hi + f;
        if (pass == 0) {
            const bool ok = seg_rows_ok(r0, r1, lane, 64u, lo, hi, A.R);
            if (!__all(ok ? 1 : 0) && lane == 0) atomicOr(&L.verdict[k], V_BAD);
        }
        if (sorted && lane == 0) {
            const uint32_t key = seg_key(lo[r0], A.R);
            if (pass == 0) atomicAdd(&L.hist[key], 1u);
            else {
                const uint64_t at = atomicAdd(&L.cursor[key], 1u);
                if (at < L.cap) L.order[at] = (uint64_t)k << 32 | s;
            }
        }
    }
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

namespace {
// Item `it` of the list the accumulate kernel walks -> *k, and the rows [*r0, *r1) of its segment; false: nothing of it is accumulated (its
// read is not V_USED).  Unsorted, *k comes in as the read of an earlier item of the same wave, or as n before its first.
__device__ __forceinline__ bool long_item(const PileLongArgs &A, uint32_t S, const LongPtrs &L, bool sorted, uint64_t it, uint32_t *k, uint32_t *r0, uint32_t *r1) {
    uint32_t s;
    if (sorted) {
        const uint64_t e = L.order[it];                                    // (it < P[n] <= cap)
        *k = (uint32_t)(e >> 32);
        s = (uint32_t)e;
        if (*k >= A.n) return false;
    } else {
        *k = *k < A.n ? seg_next(L.P, A.n, *k, it) : seg_find(L.P, A.n, it);
        s = (uint32_t)(it - L.P[*k]);
    }
    const uint32_t Q = A.qlen[*k];
    if (L.verdict[*k] != V_USED || Q > LONG_QMAX || s >= segs_of(Q, S)) return false;   // (the last two cannot be: the list was made of P)
    seg_rows(Q, S, s, r0, r1);
    return true;
}
}  // namespace

// per workgroup a slice of the (ordered) segments, a wave per segment at a time; cols as in k_pileup
__global__ __launch_bounds__(s5::NT) void k_pileup_long_accum(PileLongArgs A, uint32_t S, LongPtrs L, uint32_t sort, uint32_t cols) {
    extern __shared__ __attribute__((aligned(16))) uint64_t pile_win[];   // cols columns of COL_WORDS words
    __shared__ uint32_t s_lo;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t t = threadIdx.x; t < cols * COL_WORDS; t += s5::NT) pile_win[t] = t % COL_WORDS == 5 ? EMPTY_MINMAX : 0ull;
    if (threadIdx.x == 0) s_lo = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t total = L.P[A.n];
    const bool sorted = sort && total <= L.cap;
    uint64_t base, end;
    slice_of(total, blockIdx.x, gridDim.x, &base, &end);
    // the anchor: the smallest first lo of the segments the four waves meet first (where it lies changes the time, never the result)
    uint32_t k = A.n, r0, r1;
    if (cols && base + wave < end && long_item(A, S, L, sorted, base + wave, &k, &r0, &r1)) {
        const int32_t l0 = A.lo[A.first[k] + r0];
        if (lane == 0 && l0 >= 0 && (uint32_t)l0 < A.R) atomicMin(&s_lo, (uint32_t)l0);
    }
    __syncthreads();
    Window W;
    W.lo = s_lo == 0xFFFFFFFFu ? 0u : s_lo;
    W.cols = cols;
    s5gpu_pile_col_t *win = reinterpret_cast<s5gpu_pile_col_t *>(pile_win);
    uint64_t *head = reinterpret_cast<uint64_t *>(A.acc);
    s5gpu_pile_col_t *table = reinterpret_cast<s5gpu_pile_col_t *>(head + HEAD_WORDS);
    uint64_t cells = 0, cost = 0;                                          // this lane's
    k = A.n;
    for (uint64_t it = base + wave; it < end; it += s5::NW) {
        if (!long_item(A, S, L, sorted, it, &k, &r0, &r1)) continue;       // (the wave's branch)
        const uint64_t f = A.first[k];
        seg_cells<DevOps>(r0, r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, A.events ? A.events + f + A.ev_skip : nullptr, A.ref, A.R, W, win, table,
                          &cells, &cost);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < cols; b += s5::NT) {               // the flush: the non-empty columns of the window
        const uint32_t j = W.lo + b;
        if (j >= W.lo && j < A.R) col_merge<DevOps>(table + j, win + b);
    }
    // the reads, once each
    uint64_t used = 0, skipped = 0, bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; k < A.n; k += (uint64_t)gridDim.x * s5::NT) {
        const uint32_t v = L.verdict[k];
        if (v & V_SKIPPED) skipped++;
        else if (v & V_BAD) bad++;
        else used++;
    }
    used = wave_sum(used);
    skipped = wave_sum(skipped);
    bad = wave_sum(bad);
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

// ---------------------------------------------------------------------------------------------------------------- level histograms (§4.23)
// k_pile_hist_accum: k_pileup_long_accum's walk over the same (ordered) segments and verdicts, into R columns of 64 32-bit bins: a wave per
// segment at a time, lanes over rows, one add per cell.  The window is `cols` columns of 256 bytes in LDS (32-bit LDS adds), flushed word by
// word at the end; cells outside it are 32-bit global atomic adds.  Rules 2, 3, 5 to 11 above hold as they stand; the bin is clamped below
// 64 (hist_bin) and masked where it indexes (hist_col_add); q0 and shift are read from the head the reset wrote, the shift clamped.
namespace {
struct HistOps {
    static __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void add32_win(uint32_t *p, uint32_t v) { atomicAdd(p, v); }   // (a pointer into LDS: a ds add)
};
}  // namespace

__global__ __launch_bounds__(s5::NT) void k_pile_hist_accum(PileLongArgs A, uint32_t S, LongPtrs L, uint32_t sort, uint32_t cols, uint32_t *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist_win[];    // cols columns of HIST_BINS words: all of the 64 KB at cols = 256
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t t = threadIdx.x; t < cols * HIST_BINS; t += s5::NT) hist_win[t] = 0u;
    const uint64_t total = L.P[A.n];
    const bool sorted = sort && total <= L.cap;
    uint64_t base, end;
    slice_of(total, blockIdx.x, gridDim.x, &base, &end);
    // the anchor of k_pileup_long_accum: the smallest first lo of the segments the four waves meet first.  Every thread works it out for
    // itself (four items), so that no static LDS is needed beside the window.
    uint32_t k, r0, r1, anchor = 0xFFFFFFFFu;
    for (uint32_t w = 0; cols && w < (uint32_t)s5::NW && base + w < end; w++) {
        k = A.n;
        if (!long_item(A, S, L, sorted, base + w, &k, &r0, &r1)) continue;
        const int32_t l0 = A.lo[A.first[k] + r0];
        if (l0 >= 0 && (uint32_t)l0 < A.R && (uint32_t)l0 < anchor) anchor = (uint32_t)l0;
    }
    Window W;
    W.lo = anchor == 0xFFFFFFFFu ? 0u : anchor;
    W.cols = cols;
    const int32_t q0 = (int32_t)hist[9];                                   // s5gpu_pile_hist_head_t::q0, ::shift (32-bit words 9 and 10): written by the reset only
    const uint32_t shift = hist[10];
    uint32_t *table = hist + HIST_HEAD_WORDS;
    uint64_t *head = reinterpret_cast<uint64_t *>(hist);
    __syncthreads();
    uint64_t cells = 0;                                                    // this lane's
    k = A.n;
    for (uint64_t it = base + wave; it < end; it += s5::NW) {
        if (!long_item(A, S, L, sorted, it, &k, &r0, &r1)) continue;       // (the wave's branch)
        const uint64_t f = A.first[k];
        hist_seg_cells<HistOps>(r0, r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, q0, shift, A.R, W, hist_win, table, &cells);
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < cols * HIST_BINS; t += s5::NT) hist_flush_word<HistOps>(t, W, hist_win, table, A.R);
    // the reads, once each
    uint64_t used = 0, skipped = 0, bad = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; r < A.n; r += (uint64_t)gridDim.x * s5::NT) {
        const uint32_t v = L.verdict[r];
        if (v & V_SKIPPED) skipped++;
        else if (v & V_BAD) bad++;
        else used++;
    }
    used = wave_sum(used);
    skipped = wave_sum(skipped);
    bad = wave_sum(bad);
    cells = wave_sum(cells);
    if (lane == 0) {
        if (cells) DevOps::add64(head + 0, cells);
        if (used) DevOps::add64(head + 1, used);
        if (skipped) DevOps::add64(head + 2, skipped);
        if (bad) DevOps::add64(head + 3, bad);
    }
}

// ---------------------------------------------------------------------------------------------------------------- refine, whole reads (§4.24)
// The fit of §4.20 along the ragged paths, behind the plan and the check above (no sort: there is no window to keep warm, the segments are
// walked in P's order), and the bookkeeping of the rounds of s5gpu_extend_refine_dev:
//   k_path_fit_long    : a wave per segment, each wave a slice of consecutive segments, lanes over rows.  A lane keeps its six partial sums
//                        while the wave stays in one read; where the read changes (and at the end) the wave reduces them with shuffles and
//                        lane 0 adds them to the read's Sums with 64-bit atomics: integers, so the bytes depend on nothing but the cells
//   k_fit_long_solve   : a lane per read: verdict and sums -> fit and status (refk::long_fit_status)
//   k_requant_long     : over the same segments: q' = requant_one(q0) for the rows of the reads whose fit's status is 0
//   k_refine_long_gate : a lane per read: the status of a result row as a word of its own (what the plan and the band call read)
//   k_refine_long_round: over the same segments the rows of q, lo and hi a read takes over (refk::long_round_rule), and a lane per read its
//                        row, fit, rounds and status.  The statuses are read from one array and written to another: no wave reads what
//                        another writes.
// Rules 2, 3 (per row), 6 to 9 and 11 hold as they stand: nothing of a read is summed, requantised or copied unless its verdict is V_USED
// behind the check pass (in round 0 that of the path that came in), so first[k] + i lies inside the ragged arrays for i < Q; ref[j] is read
// behind j < R (row_sums); a[], b[] and the statuses are read at [read] for read < n.  No barrier, no LDS; branches on a read's fate are
// wave-uniform, and every shuffle is executed by all 64 lanes.
namespace {
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
// the slice of the segments (in P's order) of this wave
__device__ __forceinline__ void wave_slice(const PileLongArgs &A, const LongPtrs &L, uint64_t *g, uint64_t *end) {
    slice_of(L.P[A.n], (uint64_t)blockIdx.x * s5::NW + (threadIdx.x >> 6), (uint64_t)gridDim.x * s5::NW, g, end);
}
// segment g of the slice -> its read *k (from the read of the segment before) and, behind `true`, its rows [*r0, *r1)
__device__ __forceinline__ bool wave_seg(const PileLongArgs &A, uint32_t S, const LongPtrs &L, uint64_t g, uint32_t *k, uint32_t *r0, uint32_t *r1) {
    *k = seg_next(L.P, A.n, *k, g);
    const uint32_t Q = A.qlen[*k], s = (uint32_t)(g - L.P[*k]);
    if (Q > LONG_QMAX || s >= segs_of(Q, S)) return false;                 // (cannot be: P was made of these)
    seg_rows(Q, S, s, r0, r1);
    return true;
}
}  // namespace

__global__ __launch_bounds__(s5::NT) void k_path_fit_long(PileLongArgs A, uint32_t S, LongPtrs L, refk::Sums *sums) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t g, end;
    wave_slice(A, L, &g, &end);
    uint32_t k = g < end ? seg_find(L.P, A.n, g) : 0u, held = A.n, r0, r1;
    refk::Sums acc = {0, 0, 0, 0, 0, 0};
    for (; g < end; g++) {
        if (!wave_seg(A, S, L, g, &k, &r0, &r1) || L.verdict[k] != V_USED) continue;   // (the wave's branch)
        if (k != held) { fit_flush(sums, held, A.n, acc, lane); held = k; }
        const uint64_t f = A.first[k];
        refk::seg_sums(r0, r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, A.ref, A.R, acc);
    }
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
    uint64_t g, end;
    wave_slice(A, L, &g, &end);
    uint32_t k = g < end ? seg_find(L.P, A.n, g) : 0u, r0, r1;
    for (; g < end; g++) {
        if (!wave_seg(A, S, L, g, &k, &r0, &r1) || L.verdict[k] != V_USED || fit_status[k] != 0) continue;   // (the wave's branch)
        const uint64_t f = A.first[k];
        const double a = fit[k].a, b = fit[k].b;
        for (uint32_t i = r0 + lane; i < r1; i += 64u) out[f + i] = refk::requant_one(A.queries[f + i], a, b, clip);
    }
}

__global__ __launch_bounds__(s5::NT) void k_refine_long_gate(uint32_t n, const s5gpu_ext_row_t *__restrict__ rows, int32_t *__restrict__ st) {
    const uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x;
    if (k < n) st[k] = rows[k].status;
}

__global__ __launch_bounds__(s5::NT) void k_refine_long_round(refk::RoundLongArgs B, uint32_t round, uint32_t S, LongPtrs L) {
    const PileLongArgs &A = B.A;
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t g, end;
    wave_slice(A, L, &g, &end);
    uint32_t k = g < end ? seg_find(L.P, A.n, g) : 0u, r0, r1;
    for (; g < end; g++) {
        if (!wave_seg(A, S, L, g, &k, &r0, &r1)) continue;                 // (the wave's branch, as those below)
        const uint32_t v = L.verdict[k];
        if ((v & V_SKIPPED) || (round == 0 && v != V_USED)) continue;      // (a bad path that came in: the fills hold "no result" already)
        int32_t st;
        const int mode = refk::long_round_rule(round, v, A.qlen[k], B.cur_in[k], round ? B.t_sf[k] : 0, round ? B.t_rows[k].status : 0, &st);
        if (mode == 0) continue;
        const uint64_t f = A.first[k];                                     // (the read has segments: its layout passed this round's plan)
        for (uint32_t i = r0 + lane; i < r1; i += 64u) {
            int16_t q = 0;
            int32_t l = -1, h = -1;
            if (mode == 1) { q = A.queries[f + i]; l = A.lo[f + i]; h = A.hi[f + i]; }
            if (mode == 2) { q = B.t_q[f + i]; l = B.t_lo[f + i]; h = B.t_hi[f + i]; }
            B.q[f + i] = q; B.lo[f + i] = l; B.hi[f + i] = h;
        }
    }
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

namespace {
uint32_t g_refine_passes = 63;          // option "refine_long_passes"
uint32_t g_hist_cols = HIST_MAX_COLS;   // option "pile_hist_cols"
uint32_t g_hist_grid = MAX_GRID;        // option "pile_hist_grid"

int set_option_long(const char *key, long value) {
    const bool pow2 = value > 0 && (value & (value - 1)) == 0;
    if (strcmp(key, "pile_hist_cols") == 0 && (value == 0 || (pow2 && value >= (long)HIST_MIN_COLS && value <= (long)HIST_MAX_COLS))) {
        g_hist_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pile_hist_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_hist_grid = (uint32_t)value; return S5GPU_OK; }
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
    // which kernels the whole-read fit and its rounds launch (§4.24): 1 the plan and the check, 2 the sums, 4 the solve, 8 the requantiser,
    // 16 the bookkeeping of the rounds, 32 the band call, over what an earlier call left; 63 all (the default).  For
    // tools/extend_refine_time.py: the passes are timed apart.
    if (strcmp(key, "refine_long_passes") == 0 && value >= 1 && value <= 63) { g_refine_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

// the places of a ragged call's work area
LongPtrs long_ptrs(const PileLongArgs &A) {
    const LongWork w = long_work(A.n, A.total_rows);
    uint8_t *wk = (uint8_t *)A.work;
    LongPtrs L;
    L.verdict = (uint32_t *)(wk + w.o_verdict); L.P = (uint64_t *)(wk + w.o_prefix); L.hist = (uint32_t *)(wk + w.o_hist);
    L.cursor = (uint32_t *)(wk + w.o_cursor); L.order = (uint64_t *)(wk + w.o_order); L.cap = long_order_cap(A.n, A.total_rows);
    return L;
}
// the workgroups of a walk over the segments of a well-formed layout: four segments each at a time, `most` workgroups at most
uint32_t long_grid(const PileLongArgs &A, uint32_t S, uint32_t most) {
    const uint64_t segs = A.total_rows / S + A.n, quads = (segs + 3u) / 4u;
    return (uint32_t)(quads < most ? quads : most);
}
}  // namespace

int pilek::launch_pileup_long(const PileLongArgs &A, hipStream_t st) { return launch_pileup_long(A, nullptr, st); }

int pilek::launch_pileup_long(const PileLongArgs &A, void *hist, hipStream_t st) {
    if (A.n == 0) return S5GPU_OK;
    const uint32_t S = g_long_seg, cols = g_long_cols;
    const LongPtrs L = long_ptrs(A);
    // (the sort's counts are 32-bit: a list that 2^32 segments might not fit is walked in P's order)
    const uint32_t sort = g_long_sort && L.cap < ((uint64_t)1 << 32) ? 1u : 0u;
    const uint64_t most = A.total_rows / S + A.n, quads = (most + 3u) / 4u;  // the segments of a well-formed layout, at most
    const uint32_t grid = (uint32_t)(quads < g_long_grid ? quads : g_long_grid);
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
    if ((passes & 4u) && hist) {
        const uint32_t hcols = g_hist_cols, hgrid = (uint32_t)(quads < g_hist_grid ? quads : g_hist_grid);
        hipLaunchKernelGGL(k_pile_hist_accum, dim3(hgrid), dim3(s5::NT), (size_t)hcols * HIST_BINS * sizeof(uint32_t), st, A, S, L, sort, hcols,
                           reinterpret_cast<uint32_t *>(hist));
        S5_LAUNCH_CHECK("k_pile_hist_accum");
    }
    return S5GPU_OK;
}

// ---------------------------------------------------------------------------------------------------------------- refine, whole reads (§4.24)

uint32_t refk::long_passes() { return g_refine_passes; }

int refk::launch_long_verdicts(const PileLongArgs &A, hipStream_t st) {
    if (A.n == 0 || !(g_refine_passes & 1u)) return S5GPU_OK;
    const uint32_t S = g_long_seg;
    const LongPtrs L = long_ptrs(A);
    hipLaunchKernelGGL(k_pileup_long_plan, dim3(1), dim3(s5::NT), 0, st, A, S, L);
    S5_LAUNCH_CHECK("k_pileup_long_plan");
    hipLaunchKernelGGL(k_pileup_long_check, dim3(long_grid(A, S, g_long_grid)), dim3(s5::NT), 0, st, A, S, L, 0u, 0u);
    S5_LAUNCH_CHECK("k_pileup_long_check");
    return S5GPU_OK;
}

int refk::launch_fit_long(const FitLongArgs &F, hipStream_t st) {
    const PileLongArgs &A = F.A;
    if (A.n == 0) return S5GPU_OK;
    int rc;
    if ((rc = launch_long_verdicts(A, st))) return rc;
    const uint32_t S = g_long_seg, grid = long_grid(A, S, g_long_grid), per_read = (uint32_t)(((uint64_t)A.n + s5::NT - 1) / s5::NT);
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
    const uint32_t S = g_long_seg;
    hipLaunchKernelGGL(k_refine_long_round, dim3(long_grid(B.A, S, g_long_grid)), dim3(s5::NT), 0, st, B, round, S, long_ptrs(B.A));
    S5_LAUNCH_CHECK("k_refine_long_round");
    return S5GPU_OK;
}
