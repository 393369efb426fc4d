// pileup_dev.h — what pileup_kernels.hip and pileup_api.hip share (docs/codecs.md §4.18): the validation of a read's path, the cells of one
// query row added to a column table, the window of columns a workgroup keeps in LDS, and the launchers.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of dtw_dev.h): tests/test_pileup.py compiles it for the CPU and
// runs the very code a lane runs, with plain adds in place of the atomics, against the restatement, without a device.
#pragma once
#include <stdint.h>

#include "../../include/slow5gpu.h"

#ifdef S5_PILEUP_HOST
#define PILE_HD static inline
#else
#include <hip/hip_runtime.h>
#define PILE_HD __host__ __device__ __forceinline__
#endif

namespace pilek {

constexpr uint32_t QMAX = 1024;              // rows of the largest query (dtwk::QMAX)
constexpr uint32_t RMAX = 1u << 26;          // columns of the largest table: 3 GiB
constexpr uint32_t MIN_COLS = 64, MAX_COLS = 1024;   // the LDS window: 48 bytes a column
constexpr uint32_t MAX_GRID = 1024;
constexpr uint32_t HEAD_WORDS = 8, COL_WORDS = 6;    // 64-bit words of the totals row and of a column
constexpr uint64_t EMPTY_MINMAX = (uint64_t)32767u | ((uint64_t)(uint32_t)-32768 << 32);   // word 5 of an empty column: min_q | max_q

static_assert(sizeof(s5gpu_pile_col_t) == 8 * COL_WORDS && sizeof(s5gpu_pile_total_t) == 8 * HEAD_WORDS, "include/slow5gpu.h fixes these layouts");

// the rows of a read that count: qlen clamped to the pitch and to QMAX
PILE_HD uint32_t rows_of(uint32_t qlen, uint32_t qpitch) {
    const uint32_t q = qlen < qpitch ? qlen : qpitch;
    return q < QMAX ? q : QMAX;
}

// Row i of a read: 0 <= lo <= hi < R, and behind row 0 lo - hi_prev in {0, 1} (hi_prev = hi[i - 1]: whatever it holds, its own row's check
// decides on it; the difference is taken in 64 bits).  A read is used iff every row i < Q passes.
PILE_HD bool row_ok(uint32_t i, int32_t lo, int32_t hi, int32_t hi_prev, uint32_t R) {
    if (lo < 0 || lo > hi || (uint32_t)hi >= R) return false;
    if (i == 0) return true;
    const int64_t d = (int64_t)lo - (int64_t)hi_prev;
    return d == 0 || d == 1;
}

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

#ifndef S5_PILEUP_HOST
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
