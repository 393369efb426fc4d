// ragged_dev.h — whole reads (docs/codecs.md §4.22): the ragged layout of s5gpu_sdtw_band_dev, the work area of a call over it, and THE walk
// over its segments that every whole-read kernel takes: those of the pileup (pileup_kernels.hip), of the level histograms
// (contrast_kernels.hip, §4.23), of refine (refine_long_kernels.hip, §4.24) and of the site matrix (sites_kernels.hip, §4.25).  pileup_dev.h
// includes this file.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of dtw_dev.h): tests/test_pileup_long.py, tests/test_contrast.py and
// tests/test_extend_refine.py compile it for the CPU and resolve their segments through seg_item, the very code a lane runs.
// Values read from memory form addresses here (first, qlen, P, the ordered list).  The rules, numbered on from 1 - 6 of pileup_kernels.hip;
// the kernel files refer to them by number:
//   7. first, qlen and status are read at [read] (first also at [read + 1]) for read < n; a read has segments only behind long_verdict:
//      first[k] + Q + ev_skip <= first[k + 1] <= total_rows, Q <= 2^20, so queries, lo, hi at [first[k] + i] and events at
//      [first[k] + ev_skip + i] are inside their arrays for every i < Q, and hi[first[k] + i - 1] for 0 < i;
//   8. trip counts come from qlen, R, S, n and total_rows: a segment has at most S rows, segment numbers run below P[n], the sum of
//      ceil(Q / S), and a step from one segment's read to the next's takes at most n trips in all;
//   9. nothing of a read is accumulated unless k_pileup_long_check has passed every row of every one of its segments;
//  10. the sort's key is clamped below LONG_KEYS and indexes the counts only; a position in the ordered list is used behind `< cap`, and
//      a list that would not fit (P[n] > cap: only a layout whose reads overlap) is not made: the segments are then walked in P's order;
//  11. branches on a read's or a segment's fate are wave-uniform: they depend on values every lane of the wave reads from the same address.
// seg_item is where 7, 8 and 10 turn an item into a read and rows: no kernel does that for itself.
#pragma once
#if defined(S5_PILEUP_HOST) && !defined(S5_DTW_HOST)
#define S5_DTW_HOST
#endif
#include "dtw_dev.h"
#ifndef S5_PILEUP_HOST
#include "dev_common.h"
#endif

#define PILE_HD DTW_HD

namespace pilek {

// Row i of a read (rule 1 of pileup_kernels.hip): 0 <= lo <= hi < R, and behind row 0 lo - hi_prev in {0, 1} (hi_prev = hi[i - 1]: whatever
// it holds, its own row's check decides on it; the difference is taken in 64 bits).  A read is used iff every row i < Q passes.
PILE_HD bool row_ok(uint32_t i, int32_t lo, int32_t hi, int32_t hi_prev, uint32_t R) {
    if (lo < 0 || lo > hi || (uint32_t)hi >= R) return false;
    if (i == 0) return true;
    const int64_t d = (int64_t)lo - (int64_t)hi_prev;
    return d == 0 || d == 1;
}

// The ragged layout: read k's rows at [first[k], first[k] + qlen[k]) of queries, lo and hi.  The unit of work is a segment of S consecutive
// rows of one read.  A read's verdict is a word: 0 used (so far), SKIPPED, or BAD (ORed in by any of its segments).
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
// the places of a ragged call's work area
struct LongPtrs {
    uint32_t *verdict;               // [n]
    uint64_t *P;                     // [n + 1]
    uint32_t *hist, *cursor;         // [LONG_KEYS] each
    uint64_t *order;                 // [cap]: read << 32 | segment
    uint64_t cap;
};
PILE_HD LongPtrs long_ptrs(const PileLongArgs &A) {
    const LongWork w = long_work(A.n, A.total_rows);
    uint8_t *wk = (uint8_t *)A.work;
    LongPtrs L;
    L.verdict = (uint32_t *)(wk + w.o_verdict); L.P = (uint64_t *)(wk + w.o_prefix); L.hist = (uint32_t *)(wk + w.o_hist);
    L.cursor = (uint32_t *)(wk + w.o_cursor); L.order = (uint64_t *)(wk + w.o_order); L.cap = long_order_cap(A.n, A.total_rows);
    return L;
}

// A segment: read k, its segment s, the rows [r0, r1) of the read.  A walker starts from seg_none(n): "no read yet".
struct Seg { uint32_t k, s, r0, r1; };
PILE_HD Seg seg_none(uint32_t n) { Seg g = {n, 0u, 0u, 0u}; return g; }
// THE resolver.  Item `it` < P[n] of a walk: of the ordered list when `ordered` says that one was made (it is, iff the sort is on and
// P[n] <= cap), else of P's order.  g->k comes in as the read of an earlier item of the same walker, or as n (or more) before its first;
// in P's order the read is then stepped to from there, else found.  -> true with *g, or false: the item stands for no rows (on a work area
// the plan and the sort made that cannot be; the guards are those of rules 7, 8 and 10, and a segment that fails one is passed over, never
// clamped into place).  The read's verdict is the caller's to test.
PILE_HD bool seg_item(const PileLongArgs &A, uint32_t S, const LongPtrs &L, bool ordered, uint64_t it, Seg *g) {
    uint64_t s;
    if (ordered) {
        if (it >= L.cap) { g->k = A.n; return false; }
        const uint64_t e = L.order[it];
        g->k = (uint32_t)(e >> 32);
        s = (uint32_t)e;
        if (g->k >= A.n) return false;
    } else {
        g->k = g->k < A.n ? seg_next(L.P, A.n, g->k, it) : seg_find(L.P, A.n, it);
        if (g->k >= A.n) return false;                                     // (n = 0)
        s = it - L.P[g->k];
    }
    const uint32_t Q = A.qlen[g->k];
    if ((Q > LONG_QMAX) | (s >= segs_of(Q, S))) return false;              // (one branch: qlen and P are loaded side by side)
    g->s = (uint32_t)s;
    seg_rows(Q, S, g->s, &g->r0, &g->r1);
    return true;
}

#ifndef S5_PILEUP_HOST
// ---------------------------------------------------------------------------------------------------------------- the walks of the kernels
// Two slices, because they fix the speed: a wave's own run of consecutive segments in P's order (a read's segments stay with one wave:
// what k_path_fit_long holds its sums for), and a workgroup's run of the (ordered) list that its four waves take turn by turn (the
// neighbours of the sort stay with one LDS window).  A body runs wave-uniformly (rule 11): it may shuffle, and every shuffle is executed by
// all 64 lanes.  There is no barrier inside a walk.

// this thread's wave of its workgroup, as the scalar it is: what is indexed by it is loaded once for the wave
__device__ __forceinline__ uint32_t wave_of_group() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// the slice [*b, *e) of `total` items that part `who` of `parts` takes
__device__ __forceinline__ void slice_of(uint64_t total, uint64_t who, uint64_t parts, uint64_t *b, uint64_t *e) {
    const uint64_t per = (total + parts - 1u) / parts;
    *b = who * per < total ? who * per : total;
    *e = *b + per < total ? *b + per : total;
}

// body(const Seg &) for every segment of this wave's slice, in P's order
template <class Body>
__device__ __forceinline__ void walk_by_wave(const PileLongArgs &A, uint32_t S, const LongPtrs &L, Body body) {
    uint64_t it, end;
    slice_of(L.P[A.n], (uint64_t)blockIdx.x * s5::NW + wave_of_group(), (uint64_t)gridDim.x * s5::NW, &it, &end);
    Seg g = seg_none(A.n);
    for (; it < end; it++)
        if (seg_item(A, S, L, false, it, &g)) body(g);                     // (the wave's branch)
}

// the slice of a workgroup, of the ordered list where there is one
struct GroupSlice { uint64_t base, end; bool ordered; };
__device__ __forceinline__ GroupSlice group_slice(const PileLongArgs &A, const LongPtrs &L, uint32_t sort) {
    GroupSlice G;
    const uint64_t total = L.P[A.n];
    G.ordered = sort && total <= L.cap;
    slice_of(total, blockIdx.x, gridDim.x, &G.base, &G.end);
    return G;
}
// body(const Seg &) for items base + wave, base + wave + 4, ... of the slice
template <class Body>
__device__ __forceinline__ void walk_by_group(const PileLongArgs &A, uint32_t S, const LongPtrs &L, const GroupSlice &G, Body body) {
    Seg g = seg_none(A.n);
    for (uint64_t it = G.base + wave_of_group(); it < G.end; it += s5::NW)
        if (seg_item(A, S, L, G.ordered, it, &g)) body(g);                 // (the wave's branch)
}
// Where a workgroup's window of columns starts: the smallest first lo of the used segments its four waves meet first (where it lies
// changes the time, never the result), over the waves [w0, w1); ANCHOR_NONE if they give none, and the window then starts at column 0.
// (0, 4): every thread works it out for itself, four items: no LDS, no barrier (k_pile_hist_accum).  (wave, wave + 1): a wave's own first
// item; the workgroup takes the smallest through LDS (k_pileup_long_accum, which is measurably slower with four items a thread:
// profiles/ragged_walk_time.txt).
constexpr uint32_t ANCHOR_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t group_anchor(const PileLongArgs &A, uint32_t S, const LongPtrs &L, const GroupSlice &G, uint32_t w0, uint32_t w1) {
    uint32_t anchor = ANCHOR_NONE;
    for (uint32_t w = w0; w < w1 && G.base + w < G.end; w++) {
        Seg g = seg_none(A.n);
        if (!seg_item(A, S, L, G.ordered, G.base + w, &g) || L.verdict[g.k] != V_USED) continue;
        const int32_t l0 = A.lo[A.first[g.k] + g.r0];
        if (l0 >= 0 && (uint32_t)l0 < A.R && (uint32_t)l0 < anchor) anchor = (uint32_t)l0;
    }
    return anchor;
}
#endif

}  // namespace pilek
