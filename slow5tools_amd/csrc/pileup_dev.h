// pileup_dev.h — what pileup_kernels.hip and pileup_api.hip share (docs/codecs.md §4.18): the validation of a read's path, the cells of one
// query row added to a column table, the window of columns a workgroup keeps in LDS, and the launchers.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of dtw_dev.h): tests/test_pileup.py and tests/test_pileup_long.py
// compile it for the CPU and run the very code a lane runs, with plain adds in place of the atomics, against the restatements, without a
// device.
#pragma once
#if defined(S5_PILEUP_HOST) && !defined(S5_DTW_HOST)
#define S5_DTW_HOST
#endif
#include "dtw_dev.h"

#define PILE_HD DTW_HD

namespace pilek {

using dtwk::QMAX;                            // rows of the largest query
using dtwk::rows_of;                         // the rows of a read that count: qlen clamped to the pitch and to QMAX
constexpr uint32_t RMAX = 1u << 26;          // columns of the largest table: 3 GiB
constexpr uint32_t MIN_COLS = 64, MAX_COLS = 1024;   // the LDS window: 48 bytes a column
constexpr uint32_t MAX_GRID = 1024;
constexpr uint32_t HEAD_WORDS = 8, COL_WORDS = 6;    // 64-bit words of the totals row and of a column
constexpr uint64_t EMPTY_MINMAX = (uint64_t)32767u | ((uint64_t)(uint32_t)-32768 << 32);   // word 5 of an empty column: min_q | max_q

static_assert(sizeof(s5gpu_pile_col_t) == 8 * COL_WORDS && sizeof(s5gpu_pile_total_t) == 8 * HEAD_WORDS, "include/slow5gpu.h fixes these layouts");

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

// ---------------------------------------------------------------------------------------------------------------- whole reads (§4.22)
// The ragged layout of s5gpu_sdtw_band_dev: read k's rows at [first[k], first[k] + qlen[k]) of queries, lo and hi.  The unit of work is a
// segment of S consecutive rows of one read.  A read's verdict is a word: 0 used (so far), SKIPPED, or BAD (ORed in by any of its segments).
constexpr uint32_t LONG_QMAX = 1u << 20;     // rows of the longest read (bandk::EMAX)
constexpr uint32_t SEG_MIN = 64, SEG_MAX = 1024;
constexpr uint32_t LONG_KEYS = 1024;         // buckets of the segments' counting sort
constexpr uint64_t LONG_ROWS_MAX = (uint64_t)1 << 40;
constexpr uint32_t V_USED = 0, V_SKIPPED = 1, V_BAD = 2;

// the layout checks of read k: f0 = first[k], f1 = first[k + 1].  Behind V_USED every row i < Q of the read, and its event row
// first[k] + ev_skip + i, lies inside [0, total_rows).
PILE_HD uint32_t long_verdict(uint64_t f0, uint64_t f1, uint32_t Q, int32_t status, uint64_t total_rows, uint32_t ev_skip) {
    if (status != 0 || Q == 0) return V_SKIPPED;
    if (Q > LONG_QMAX || f0 > f1 || f1 > total_rows || (uint64_t)Q + ev_skip > f1 - f0) return V_BAD;
    return V_USED;
}
PILE_HD uint32_t segs_of(uint32_t Q, uint32_t S) { return (Q + S - 1u) / S; }          // (Q <= 2^20)
// the rows [*r0, *r1) of segment s < segs_of(Q, S)
PILE_HD void seg_rows(uint32_t Q, uint32_t S, uint32_t s, uint32_t *r0, uint32_t *r1) {
    *r0 = s * S;
    *r1 = Q - *r0 < S ? Q : *r0 + S;
}
// The segments are numbered along P, the [n + 1] exclusive prefix of the reads' segments (none for a read that is not V_USED after the
// layout checks): segment g < P[n] belongs to the one read k with P[k] <= g < P[k + 1], as its segment g - P[k].  At most 32 trips.
PILE_HD uint32_t seg_find(const uint64_t *P, uint32_t n, uint64_t g) {
    uint32_t a = 0, b = n;
    for (uint32_t t = 0; t < 32u && b - a > 1u; t++) {
        const uint32_t mid = a + (b - a) / 2u;
        if (P[mid] <= g) a = mid; else b = mid;
    }
    return a;
}
// ... and from a read k0 at or before it: at most n trips
PILE_HD uint32_t seg_next(const uint64_t *P, uint32_t n, uint32_t k0, uint64_t g) {
    uint32_t k = k0;
    while (k + 1u < n && P[k + 1u] <= g) k++;
    return k;
}
// the bucket of a segment whose first row starts at column lo0 (unvalidated: the key is clamped and orders the work, nothing else)
PILE_HD uint32_t seg_key(int32_t lo0, uint32_t R) {
    const uint32_t block = (R + LONG_KEYS - 1u) / LONG_KEYS;               // >= 1
    const uint32_t key = lo0 < 0 ? 0u : (uint32_t)lo0 / block;
    return key < LONG_KEYS ? key : LONG_KEYS - 1u;
}
// Rows r0 + lane, r0 + lane + step, ... < r1 of a read whose lo, hi (and q, ev) point at ITS row 0: hi_prev of a row is the row before it in
// the ragged array, whichever segment that lies in.  On the device lane < step = 64; on the host (0, 1).
PILE_HD bool seg_rows_ok(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, uint32_t R) {
    bool ok = true;
    for (uint32_t i = r0 + lane; i < r1; i += step) ok = ok && row_ok(i, lo[i], hi[i], i ? hi[i - 1] : 0, R);
    return ok;
}
template <class Ops>
PILE_HD void seg_cells(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, const int16_t *q, const s5gpu_event_t *ev,
                       const int16_t *ref, uint32_t R, const Window &W, s5gpu_pile_col_t *win, s5gpu_pile_col_t *cols, uint64_t *cells, uint64_t *cost) {
    for (uint32_t i = r0 + lane; i < r1; i += step)
        row_cells<Ops>(i, lo[i], hi[i], i ? hi[i - 1] : 0, (int32_t)q[i], ev ? ev[i].length : 0u, ref, R, W, win, cols, cells, cost);
}
// the work area of a ragged call: verdicts [n], P [n + 1], the sort's counts and cursors, and the ordered segments (a read and a segment
// each), one for every segment the smallest S makes of a layout whose reads do not overlap: the sum of ceil(Q / S) is at most this
PILE_HD uint64_t long_order_cap(uint32_t n, uint64_t total_rows) { return total_rows / SEG_MIN + n; }
PILE_HD uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
struct LongWork { uint64_t o_verdict, o_prefix, o_hist, o_cursor, o_order, bytes; };
PILE_HD LongWork long_work(uint32_t n, uint64_t total_rows) {
    LongWork w;
    w.o_verdict = 0;
    w.o_prefix = up16(4ull * n);
    w.o_hist = w.o_prefix + up16(8ull * ((uint64_t)n + 1u));
    w.o_cursor = w.o_hist + 4ull * LONG_KEYS;
    w.o_order = w.o_cursor + 4ull * LONG_KEYS;
    w.bytes = w.o_order + up16(8ull * long_order_cap(n, total_rows));
    return w;
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
struct PileLongArgs {
    uint32_t n;
    const int16_t *queries;          // [total_rows]
    const uint64_t *first;           // [n + 1]
    const uint32_t *qlen;
    uint64_t total_rows;
    const int16_t *ref;
    uint32_t R;
    const int32_t *lo, *hi;          // [total_rows]
    const int32_t *status;
    const s5gpu_event_t *events;     // [total_rows], or nullptr
    uint32_t ev_skip;                // 0 without events
    void *work;                      // long_work(n, total_rows).bytes
    void *acc;
};
// k_pileup_long_plan, _check, (the sort,) _accum over the reads of a ragged batch, on st
int launch_pileup_long(const PileLongArgs &A, hipStream_t st);
// ... and from the same verdicts and segment list k_pile_hist_accum into hist (§4.23), when hist is given; A.acc (with A.ref and A.events)
// may then be NULL: the histogram alone
int launch_pileup_long(const PileLongArgs &A, void *hist, hipStream_t st);
// k_pile_hist_reset; k reads that never reached the device count as skipped in a histogram; k_pile_contrast (contrast_kernels.hip)
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
