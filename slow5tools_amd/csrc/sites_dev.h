// sites_dev.h — what sites_kernels.hip and sites_api.hip share (docs/codecs.md §4.25): the sub-range of the site list a segment can touch, the
// cells of one query row at the sites it crosses, the level of a cell and its score row against a control column, and the launchers.
// With S5_PILEUP_HOST defined only the plain C++ is declared (the switch of pileup_dev.h): tests/test_sites.py compiles it for the CPU and
// runs the very code a lane runs, with plain adds in place of the atomics, against the restatement, without a device.
// Values read from memory form addresses here: a site index t indexes the list and the output only behind t < M, and sites[t] indexes the
// histogram only behind `< R`.  A list that is not strictly increasing only moves where the searches land inside [0, M): the counts are
// then unspecified, the accesses are not.
#pragma once
#include "pileup_dev.h"

namespace pilek {

constexpr uint32_t SITES_MAX = 1u << 16;             // sites of the longest list: 256 KB
constexpr uint64_t SITE_CELLS_MAX = 1ull << 27;      // entries of the largest matrix: 2 GiB
constexpr uint32_t SITE_ROW_NONE = 0xFFFFFFFFu;      // row0 of the empty entry

static_assert(sizeof(s5gpu_site_cell_t) == 16 && sizeof(s5gpu_site_score_t) == 16, "include/slow5gpu.h fixes these layouts");

// the smallest t in [a, b) with sites[t] >= v, or b: at most 32 trips, and what comes back lies in [a, b]
PILE_HD uint32_t site_lower(const uint32_t *sites, uint32_t a, uint32_t b, uint32_t v) {
    for (uint32_t trip = 0; trip < 32u && a < b; trip++) {
        const uint32_t mid = a + (b - a) / 2u;
        if (sites[mid] < v) a = mid + 1u; else b = mid;
    }
    return a;
}
// The sites [*sa, *sb) that rows from column lo0 up to column hi1 can cross, both validated (0 <= lo0, hi1 < R <= 2^22): sb <= M
PILE_HD void site_range(const uint32_t *sites, uint32_t M, int32_t lo0, int32_t hi1, uint32_t *sa, uint32_t *sb) {
    *sa = site_lower(sites, 0u, M, (uint32_t)lo0);
    *sb = site_lower(sites, *sa, M, (uint32_t)hi1 + 1u);
}
// One row added to an entry.  Ops: add64, add32 and min32 on the matrix's memory (atomics on the device, plain on the host).
template <class Ops>
PILE_HD void site_cell_add(s5gpu_site_cell_t *c, int32_t q, uint32_t i) {
    Ops::add64(reinterpret_cast<uint64_t *>(&c->sum_q), (uint64_t)(int64_t)q);
    Ops::add32(&c->cells, 1u);
    Ops::min32(&c->row0, i);
}
// Row i of read k, which passed row_ok with its whole read: the sites of [sa, sb) with lo <= sites[t] <= hi, at most sb - sa trips, t < M
// checked again before the list and the matrix are touched
template <class Ops>
PILE_HD void site_row_cells(uint32_t i, int32_t lo, int32_t hi, int32_t q, const uint32_t *sites, uint32_t sa, uint32_t sb, uint32_t M, uint32_t k, uint32_t n,
                            s5gpu_site_cell_t *out) {
    for (uint32_t t = site_lower(sites, sa, sb, (uint32_t)lo); t < sb && t < M && sites[t] <= (uint32_t)hi; t++) site_cell_add<Ops>(out + (uint64_t)t * n + k, q, i);
}
// The rows [r0, r1) of a segment of read k, r0 < r1, as seg_cells walks them (lo, hi and q point at the read's row 0).  The segment's first lo
// and last hi are the same two words for every lane; behind the check pass they bound every row's columns.  A segment that can touch no site
// costs those two loads and the two searches.
template <class Ops>
PILE_HD void site_seg_cells(uint32_t r0, uint32_t r1, uint32_t lane, uint32_t step, const int32_t *lo, const int32_t *hi, const int16_t *q, const uint32_t *sites,
                            uint32_t M, uint32_t k, uint32_t n, s5gpu_site_cell_t *out) {
    uint32_t sa, sb;
    site_range(sites, M, lo[r0], hi[r1 - 1u], &sa, &sb);
    if (sa >= sb) return;                                                  // (the wave's branch)
    for (uint32_t i = r0 + lane; i < r1; i += step) site_row_cells<Ops>(i, lo[i], hi[i], (int32_t)q[i], sites, sa, sb, M, k, n, out);
}

// ---------------------------------------------------------------------------------------------------------------- the score
// The level of an entry with cells > 0: floor((2 sum_q + cells) / (2 cells)), the mean rounded half up, as the floor of sum_q / cells and
// its remainder (no product: whatever sum_q holds nothing overflows).  For the cells of real reads it lies inside int16; the row keeps its
// low 16 bits.
PILE_HD int16_t site_level(int64_t sum_q, uint32_t cells) {
    const int64_t c = (int64_t)cells;
    int64_t d = sum_q / c, rem = sum_q % c;
    if (rem < 0) { d -= 1; rem += c; }                                     // the floor, for negatives too
    if (2 * rem >= c) d += 1;
    return (int16_t)(uint16_t)(uint64_t)d;
}
PILE_HD uint32_t site_sat32(uint64_t v) { return v < 0xFFFFFFFFull ? (uint32_t)v : 0xFFFFFFFFu; }
// the level and the bin of an entry, 0 and bin 0 for one without cells
PILE_HD uint32_t site_level_bin(const s5gpu_site_cell_t &c, int32_t q0, uint32_t shift, int16_t *level) {
    *level = c.cells ? site_level(c.sum_q, c.cells) : (int16_t)0;
    return c.cells ? hist_bin((int32_t)*level, q0, shift) : 0u;
}
// The row of an entry whose level falls in bin b, from the column's inclusive prefix sums at b (cum_b) and at b - 1 (cum_prev: 0 for b = 0)
// and its total n.  flags: what the column gave (0 or S5GPU_SITE_COLUMN).
PILE_HD s5gpu_site_score_t site_score_row(const s5gpu_site_cell_t &c, int16_t level, uint64_t cum_b, uint64_t cum_prev, uint64_t n, uint32_t flags) {
    s5gpu_site_score_t r;
    const bool has = c.cells != 0u;
    r.level = has ? level : (int16_t)0;
    r.flags = (uint16_t)(flags | (has ? 0u : S5GPU_SITE_NO_CELL) | (n == 0 ? S5GPU_SITE_EMPTY : 0u));
    r.below = has ? site_sat32(cum_b) : 0u;
    r.above = has ? site_sat32(n - cum_prev) : 0u;
    r.n = site_sat32(n);
    return r;
}
PILE_HD s5gpu_site_score_t site_score_head() {
    s5gpu_site_score_t r = {0, (uint16_t)S5GPU_SITE_HEAD, 0u, 0u, 0u};
    return r;
}
// does a histogram's head (its 32-bit words) agree with R and with 64 bins
PILE_HD bool site_head_ok(const uint32_t *hist, uint32_t R) { return hist[8] == R && hist[11] == HIST_BINS; }

#ifndef S5_PILEUP_HOST
// the fill, then behind launch_long_plan_check k_site_cells over the reads of a ragged batch, on st
int launch_site_cells(const PileLongArgs &A, const uint32_t *sites, uint32_t M, s5gpu_site_cell_t *out, uint32_t *verdict_out, hipStream_t st);
// k_site_score
int launch_site_score(const s5gpu_site_cell_t *cells, uint32_t n, const uint32_t *sites, uint32_t M, const void *hist, uint32_t R, s5gpu_site_score_t *out, hipStream_t st);
// "site_passes" of s5gpu_set_option (sites_kernels.hip)
int site_set_option(const char *key, long value);
#endif

}  // namespace pilek
