// pileup_dev.h — what pileup_kernels.hip and pileup_api.hip share (docs/codecs.md §4.18): the validation of a read's path, the cells of one
// query row added to a column table, the window of columns a workgroup keeps in LDS, the level histograms of §4.23, and the launchers.  The
// ragged layout of whole reads (§4.22), row_ok and the PILE_HD / S5_PILEUP_HOST switch come with ragged_dev.h.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of dtw_dev.h): tests/test_pileup.py, tests/test_pileup_long.py and
// tests/test_contrast.py compile it for the CPU and run the very code a lane runs, with plain adds in place of the atomics, against the
// restatements, without a device.
#pragma once
#include "ragged_dev.h"

namespace pilek {

using dtwk::QMAX;                            // rows of the largest query
using dtwk::rows_of;                         // the rows of a read that count: qlen clamped to the pitch and to QMAX
constexpr uint32_t RMAX = 1u << 26;          // columns of the largest table: 3 GiB
constexpr uint32_t MIN_COLS = 64, MAX_COLS = 1024;   // the LDS window: 48 bytes a column
constexpr uint32_t MAX_GRID = 1024;
constexpr uint32_t HEAD_WORDS = 8, COL_WORDS = 6;    // 64-bit words of the totals row and of a column
constexpr uint64_t EMPTY_MINMAX = (uint64_t)32767u | ((uint64_t)(uint32_t)-32768 << 32);   // word 5 of an empty column: min_q | max_q

static_assert(sizeof(s5gpu_pile_col_t) == 8 * COL_WORDS && sizeof(s5gpu_pile_total_t) == 8 * HEAD_WORDS, "include/slow5gpu.h fixes these layouts");

// The window: columns [lo, lo + cols) live in a table of their own (LDS on the device), cols 0 or a power of two.  -> is column j inside,
// and its slot there: the index is masked behind the range test, so it is inside the table whatever j is.
struct Window { uint32_t lo, cols; };
PILE_HD bool window_slot(const Window &W, uint32_t j, uint32_t *slot) {
    const uint32_t d = j - W.lo;
    *slot = d & (W.cols - 1u);
    return d < W.cols;
}

// One cell added to a column.  Ops: add64, and minmax32 on a column's min_q and max_q, on the table's memory (atomics on the device, plain
// on the host).  depth and n_events are one 64-bit word (little-endian: depth below), added at once: a column holds fewer than 2^32 cells.
template <class Ops>
PILE_HD void col_add(s5gpu_pile_col_t *c, bool first, int32_t q, uint32_t length, uint32_t cost) {
    uint64_t *w = reinterpret_cast<uint64_t *>(c);
    Ops::add64(w, (first ? 1ull : 0ull) | (1ull << 32));
    if (length) Ops::add64(w + 1, length);
    Ops::add64(w + 2, (uint64_t)(int64_t)q);
    Ops::add64(w + 3, (uint64_t)((int64_t)q * q));
    Ops::add64(w + 4, cost);
    Ops::minmax32(c, q, q);
}

// A column of a window added to the table's column (the flush), and emptied
template <class Ops>
PILE_HD void col_merge(s5gpu_pile_col_t *dst, s5gpu_pile_col_t *src) {
    uint64_t *d = reinterpret_cast<uint64_t *>(dst), *s = reinterpret_cast<uint64_t *>(src);
    if (src->n_events == 0) return;
    Ops::add64(d, s[0]);
    if (s[1]) Ops::add64(d + 1, s[1]);
    Ops::add64(d + 2, s[2]);
    Ops::add64(d + 3, s[3]);
    Ops::add64(d + 4, s[4]);
    Ops::minmax32(dst, src->min_q, src->max_q);
    s[0] = s[1] = s[2] = s[3] = s[4] = 0;
    s[5] = EMPTY_MINMAX;
}

// The cells of row i of a read that passed row_ok in EVERY row: columns lo .. hi, at most R trips, j < R checked again before ref[j] and the
// table are touched.  q: the row's query value; length: its event's samples (0: none given).  cells / cost: the caller's running totals.
template <class Ops>
PILE_HD void row_cells(uint32_t i, int32_t lo, int32_t hi, int32_t hi_prev, int32_t q, uint32_t length, const int16_t *ref, uint32_t R, const Window &W,
                       s5gpu_pile_col_t *win, s5gpu_pile_col_t *cols, uint64_t *cells, uint64_t *cost) {
    const uint32_t trips = (uint32_t)(hi - lo) + 1u;
    uint32_t j = (uint32_t)lo;
    for (uint32_t t = 0; t < trips && t < R && j < R; t++, j++) {
        const bool first = i == 0 || (int32_t)j > hi_prev;
        const int32_t d = q - (int32_t)ref[j];
        const uint32_t c = (uint32_t)(d < 0 ? -d : d);
        uint32_t slot;
        if (window_slot(W, j, &slot)) col_add<Ops>(win + slot, first, q, length, c);
        else col_add<Ops>(cols + j, first, q, length, c);
        *cells += 1;
        *cost += c;
    }
}

// the rows of a segment of a whole read (ragged_dev.h, §4.22), as seg_rows_ok walks them
template <class Ops>
PILE_HD void seg_cells(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, const int16_t *q, const s5gpu_event_t *ev,
                       const int16_t *ref, uint32_t R, const Window &W, s5gpu_pile_col_t *win, s5gpu_pile_col_t *cols, uint64_t *cells, uint64_t *cost) {
    for (uint32_t i = r0 + lane; i < r1; i += step)
        row_cells<Ops>(i, lo[i], hi[i], i ? hi[i - 1] : 0, (int32_t)q[i], ev ? ev[i].length : 0u, ref, R, W, win, cols, cells, cost);
}

// ---------------------------------------------------------------------------------------------------------------- level histograms (§4.23)
// Beside the table: R columns of 64 32-bit counts behind a head.  A column is 256 bytes, a lane per bin for one wave.
constexpr uint32_t HIST_RMAX = 1u << 22;     // columns of the largest histogram: 1 GiB
constexpr uint32_t HIST_BINS = 64, HIST_SHIFT_MAX = 10;
constexpr uint32_t HIST_MIN_COLS = 16, HIST_MAX_COLS = 256;   // the LDS window: 256 bytes a column, 64 KB at most
constexpr uint32_t HIST_HEAD_WORDS = 16;     // 32-bit words of the head

static_assert(sizeof(s5gpu_pile_hist_head_t) == 4 * HIST_HEAD_WORDS && sizeof(s5gpu_pile_contrast_t) == 40, "include/slow5gpu.h fixes these layouts");

// the bin of a level: shift comes from memory and is clamped before it shifts; the bin is below HIST_BINS whatever q, q0 and shift are
PILE_HD uint32_t hist_bin(int32_t q, int32_t q0, uint32_t shift) {
    const int64_t d = (int64_t)q - q0;
    if (d < 0) return 0u;
    const uint64_t b = (uint64_t)d >> (shift < HIST_SHIFT_MAX ? shift : HIST_SHIFT_MAX);
    return b < HIST_BINS - 1u ? (uint32_t)b : HIST_BINS - 1u;
}
// One cell added to a column's bin.  Ops: add32_win on the window's memory and add32 on the table's (atomics on the device, plain on the host).
template <class Ops>
PILE_HD void hist_col_add(uint32_t *col, uint32_t bin, bool in_window) {
    if (in_window) Ops::add32_win(col + (bin & (HIST_BINS - 1u)), 1u);
    else Ops::add32(col + (bin & (HIST_BINS - 1u)), 1u);
}
// Word t of a window of W.cols columns added to the table (the flush) and emptied; a slot that stands for no column of the table holds nothing
template <class Ops>
PILE_HD void hist_flush_word(uint32_t t, const Window &W, uint32_t *win, uint32_t *table, uint32_t R) {
    const uint32_t j = W.lo + t / HIST_BINS, v = win[t];
    if (v == 0u || j < W.lo || j >= R) return;
    Ops::add32(table + (uint64_t)j * HIST_BINS + t % HIST_BINS, v);
    win[t] = 0u;
}
// The cells of a row that passed row_ok with its whole read: columns lo .. hi, the trips and the second `j < R` of row_cells
template <class Ops>
PILE_HD void hist_row_cells(int32_t lo, int32_t hi, uint32_t bin, uint32_t R, const Window &W, uint32_t *win, uint32_t *table, uint64_t *cells) {
    const uint32_t trips = (uint32_t)(hi - lo) + 1u;
    uint32_t j = (uint32_t)lo;
    for (uint32_t t = 0; t < trips && t < R && j < R; t++, j++) {
        uint32_t slot;
        if (window_slot(W, j, &slot)) hist_col_add<Ops>(win + slot * HIST_BINS, bin, true);
        else hist_col_add<Ops>(table + (uint64_t)j * HIST_BINS, bin, false);
        *cells += 1;
    }
}
// the rows of a segment, as seg_cells
template <class Ops>
PILE_HD void hist_seg_cells(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, const int16_t *q, int32_t q0, uint32_t shift,
                            uint32_t R, const Window &W, uint32_t *win, uint32_t *table, uint64_t *cells) {
    for (uint32_t i = r0 + lane; i < r1; i += step) hist_row_cells<Ops>(lo[i], hi[i], hist_bin((int32_t)q[i], q0, shift), R, W, win, table, cells);
}

#ifndef S5_PILEUP_HOST
// What the kernels of pileup_kernels.hip, contrast_kernels.hip and refine_long_kernels.hip share beside the walks of ragged_dev.h
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
// the inclusive prefix sums of a wave's 64 values (k_pile_contrast, k_site_score: a lane per bin)
__device__ __forceinline__ uint64_t wave_incl_add64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(v, d);
        if (lane >= (uint32_t)d) v += t;
    }
    return v;
}
// the reads of a ragged batch, once each, from their verdicts: the grid's threads share them out; in every lane the wave's counts
struct ReadCounts { uint64_t used, skipped, bad; };
__device__ __forceinline__ ReadCounts verdict_counts(const uint32_t *verdict, uint32_t n) {
    ReadCounts c = {0, 0, 0};
    for (uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; k < n; k += (uint64_t)gridDim.x * s5::NT) {
        const uint32_t v = verdict[k];
        if (v & V_SKIPPED) c.skipped++;
        else if (v & V_BAD) c.bad++;
        else c.used++;
    }
    c.used = wave_sum(c.used);
    c.skipped = wave_sum(c.skipped);
    c.bad = wave_sum(c.bad);
    return c;
}
// a wave's totals v[i] added to word i of a head, by its lane 0, where they are not 0
template <int N>
__device__ __forceinline__ void head_add(uint64_t *head, const uint64_t (&v)[N]) {
    if ((threadIdx.x & 63u) != 0) return;
#pragma unroll
    for (int i = 0; i < N; i++)
        if (v[i]) DevOps::add64(head + i, v[i]);
}

// k_pileup_long_plan, _check, (the sort,) _accum over the reads of a ragged batch, on st
int launch_pileup_long(const PileLongArgs &A, hipStream_t st);
// ... and from the same verdicts and segment list k_pile_hist_accum into hist (§4.23), when hist is given; A.acc (with A.ref and A.events)
// may then be NULL: the histogram alone
int launch_pileup_long(const PileLongArgs &A, void *hist, hipStream_t st);
// the plan and the check alone (no sort): the verdicts and P in A.work, for a walk of another file (refine_long_kernels.hip)
int launch_long_plan_check(const PileLongArgs &A, hipStream_t st);
// "pileup_long_seg"; and the workgroups of a walk over the segments of a well-formed layout, four segments each at a time: at most `most`,
// or "pileup_long_grid" of them
uint32_t long_seg();
uint32_t long_grid(const PileLongArgs &A, uint32_t S, uint32_t most);
uint32_t long_grid(const PileLongArgs &A, uint32_t S);
// k_pile_hist_accum over the verdicts and the (ordered) segments launch_pileup_long left in L (contrast_kernels.hip, as the four below)
int launch_hist_accum(const PileLongArgs &A, uint32_t S, const LongPtrs &L, uint32_t sort, void *hist, hipStream_t st);
int hist_set_option(const char *key, long value);
// k_pile_hist_reset; k reads that never reached the device count as skipped in a histogram; k_pile_contrast
int launch_hist_reset(void *hist, uint32_t R, int32_t q0, uint32_t shift, hipStream_t st);
int launch_hist_add_skipped(void *hist, uint32_t k, hipStream_t st);
int launch_contrast(const void *hist_a, const void *hist_b, const void *acc_a, const void *acc_b, uint32_t R, s5gpu_pile_contrast_t *out, hipStream_t st);

struct PileArgs {
    const int16_t *queries;          // [n, qpitch]
    uint32_t qpitch;
    const uint32_t *qlen;
    const int16_t *ref;
    uint32_t R;
    const int32_t *lo, *hi;          // [n, qpitch]
    const int32_t *status;
    const s5gpu_event_t *events;     // [n, qpitch], or nullptr
    void *acc;                       // the totals row and R columns
};
// k_pileup_reset, k_pileup over n reads, and k_pileup_add_skipped (k reads that never reached the device count as skipped), on st
int launch_reset(void *acc, uint32_t R, hipStream_t st);
int launch_pileup(uint32_t n, const PileArgs &A, hipStream_t st);
int launch_add_skipped(void *acc, uint32_t k, hipStream_t st);
// s5gpu_set_option's keys of the pileup (pileup_kernels.hip)
int set_option(const char *key, long value);
#endif

}  // namespace pilek
