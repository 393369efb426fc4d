// band_dev.h — what band_kernels.hip and band_api.hip share (docs/codecs.md §4.21): the ranges of the parameters, the bookkeeping of the tiles
// (windows, the carried row, slots), the walk through the tiles, and the launchers.  The lane code is dtw_dev.h's (lane_step_dirs, lane_best).
// With S5_BAND_HOST (or S5_DTW_HOST) defined only the plain C++ is declared (the switch of dtw_dev.h): tests/test_extend.py compiles it for
// the CPU and runs the very code a lane runs against the restatement, without a device.
#pragma once
#if defined(S5_BAND_HOST) && !defined(S5_DTW_HOST)
#define S5_DTW_HOST
#endif
#include "dtw_dev.h"

namespace bandk {

using dtwk::FAR;
using dtwk::U4;

constexpr uint32_t EMAX = 1u << 20;          // rows of the longest query
constexpr uint32_t BAND_MIN = 64, BAND_MAX = 4096;
constexpr uint32_t CARRY_MAX = 1u << 29;     // a carried value is below this, or it is FAR
static_assert(sizeof(s5gpu_band_params_t) == 32 && sizeof(s5gpu_ext_row_t) == 32, "include/slow5gpu.h fixes these layouts");

// tile_rows in {64, 128, 256, 512, 1024}
DTW_HD bool tile_ok(uint32_t T) { return T == 64u || T == 128u || T == 256u || T == 512u || T == 1024u; }
// band a multiple of 64 in 64 .. 4096
DTW_HD bool band_ok(uint32_t band) { return band >= BAND_MIN && band <= BAND_MAX && (band & 63u) == 0; }
// every parameter inside the ranges of §4.21 (NaN fails every compare)
DTW_HD bool params_ok(const s5gpu_band_params_t &P) {
    return P.emin >= 1u && P.emax >= P.emin && P.emax <= EMAX && tile_ok(P.tile_rows) && band_ok(P.band) && P.clip >= 1 && P.clip <= 32767 &&
           P.scale > 0.0 && P.scale <= 1.7976931348623157e308;
}

// Q of a read with E event rows; 0: no query (QUERY_SHORT where no status came in)
DTW_HD uint32_t long_qlen(uint64_t E, uint32_t skip, uint32_t emin, uint32_t emax) {
    const uint64_t avail = E > skip ? E - skip : 0;
    const uint32_t Q = avail < emax ? (uint32_t)avail : emax;
    return Q < emin ? 0u : Q;
}

// ---------------------------------------------------------------------------------------------------------------- tiles
// the tiles of Q rows, and the rows of tile k < tiles_of(Q, T)
DTW_HD uint32_t tiles_of(uint32_t Q, uint32_t T) { return (Q + T - 1u) / T; }
DTW_HD uint32_t tile_rows_of(uint32_t Q, uint32_t T, uint32_t k) { const uint32_t left = Q - k * T; return left < T ? left : T; }
// the last first column a window may have, and the columns of the window at a <= amax
DTW_HD uint32_t win_amax(uint32_t R, uint32_t band) { return R > band ? R - band : 0u; }
DTW_HD uint32_t win_cols(uint32_t a, uint32_t R, uint32_t band) { return R - a < band ? R - a : band; }
// clamp(c - band / 4, lo, amax): the window's first column for a path at column c (lo <= amax)
DTW_HD uint32_t win_place(uint32_t c, uint32_t band, uint32_t lo, uint32_t amax) {
    const uint32_t q = band / 4u, want = c > q ? c - q : 0u;
    return want < lo ? lo : want > amax ? amax : want;
}
// the first slot of read i whose rows start at `first`, counted from the group's first row (§4.21: disjoint without a scan, since floor(x) + floor(y) <= floor(x + y))
DTW_HD uint64_t slot_first(uint64_t first, uint32_t T, uint64_t i) { return first / T + i; }
DTW_HD uint64_t slot_count(uint64_t total_rows, uint32_t T, uint64_t n) { return total_rows / T + n; }
// the scratch of slot_count slots: the slots, then an int32 per slot (the tile's first column a_k)
DTW_HD uint64_t scratch_bytes(uint64_t slots, uint32_t slot_words) { return slots * ((uint64_t)slot_words * 256u) + ((slots * 4u + 15u) & ~(uint64_t)15u); }

// The carried row lives in band + 1 words S: S[0] is "no cell" (the column left of the window), S[j + 1] the bottom cell of window column j
// of the tile before, as that tile left it.  What the next tile, whose window starts `delta` columns further right, takes for the cell above
// its window column x - 1 (x = 0: the diagonal of column 0), x <= its own width: S[delta + x] where that is a column of the tile before,
// less that tile's minimum, unless the cell is no cell or the difference reaches 2^29.  The first tile has the free start instead.
DTW_HD uint32_t carry_index(uint32_t delta, uint32_t x, uint32_t wprev, bool *in) {
    const uint32_t at = delta + x;
    *in = at <= wprev;
    return *in ? at : 0u;
}
DTW_HD uint32_t carry_value(uint32_t raw, bool in, uint32_t pmin, bool first) {
    const uint32_t v = raw - pmin;
    return first ? 0u : in && raw < FAR && v < CARRY_MAX ? v : FAR;
}

DTW_HD s5gpu_ext_row_t row_none(int32_t status) {
    s5gpu_ext_row_t r;
    r.cost = ~(uint64_t)0; r.qlen = 0; r.tiles = 0; r.start = -1; r.end = -1; r.a_last = -1; r.status = status;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- the walk
// From (Q - 1, end) along the decisions of the read's tiles to global row 0; a move out of a tile's row 0 lands in the last row of the tile
// before.  slots: the read's first slot (its tiles follow one another); tile_a[k]: the first column of tile k's window.  lo[i], hi[i]
// (i < Q) get absolute columns.  Decisions and tile_a are read from memory, so everything is bounded here, as in dtwk::path_walk_from: a
// tile has at most Qk + W_k trips (Q + sum W_k in all); i < Qk and j < W_k are checked before each use; a window has to lie in the
// reference; a word index is clamped to the slot; a code of 3 or a step out of a window ends the walk.
// -> 0 and *start_out, or S5GPU_STATUS_PATH_ROW (*start_out = -1; lo and hi hold a partial path: the caller overwrites them)
DTW_HD int32_t band_walk(const uint32_t *slots, uint32_t slot_words, const int32_t *tile_a, uint32_t G, uint32_t T, uint32_t band, uint32_t Q, uint32_t R,
                         int32_t end, int32_t *lo, int32_t *hi, int32_t *start_out) {
    *start_out = -1;
    if (Q == 0 || Q > EMAX || R == 0 || slot_words == 0 || end < 0 || (uint32_t)end >= R) return S5GPU_STATUS_PATH_ROW;
    const uint32_t top = slot_words * 64u - 1u, amax = win_amax(R, band);
    uint32_t col = (uint32_t)end;
    hi[Q - 1] = end;
    for (uint32_t k = tiles_of(Q, T); k-- > 0;) {
        const uint32_t Qk = tile_rows_of(Q, T, k);
        const int32_t a_in = tile_a[k];
        if (a_in < 0 || (uint32_t)a_in > amax) return S5GPU_STATUS_PATH_ROW;
        const uint32_t a = (uint32_t)a_in, W = win_cols(a, R, band);
        const uint32_t *words = slots + (uint64_t)k * ((uint64_t)slot_words * 64u);
        uint32_t i = Qk - 1, j = col - a, at = 0xFFFFFFFFu, word = 0;      // (col < a: far above W)
        bool out = false;
        for (uint32_t trip = 0; trip < Qk + W; trip++) {
            if (i >= Qk || j >= W) return S5GPU_STATUS_PATH_ROW;
            if (k == 0 && i == 0) {
                lo[0] = (int32_t)(a + j);
                *start_out = (int32_t)(a + j);
                return 0;
            }
            uint32_t shift;
            uint32_t x = dtwk::path_cell(G, i, j, &shift);
            x = x < top ? x : top;
            if (x != at) { word = words[x]; at = x; }
            const uint32_t code = (word >> shift) & 3u;
            if (code == 3u) return S5GPU_STATUS_PATH_ROW;
            if (code == 2u) {
                if (j == 0) return S5GPU_STATUS_PATH_ROW;
                j--;
                continue;
            }
            const uint32_t gi = k * T + i;                                 // (>= 1 here)
            col = a + j;
            lo[gi] = (int32_t)col;
            if (code == 0u) {
                if (col == 0) return S5GPU_STATUS_PATH_ROW;
                col--;
            }
            hi[gi - 1] = (int32_t)col;
            if (i == 0) { out = true; break; }                             // into the last row of tile k - 1, at col
            i--;
            j = col - a;                                                   // (left of the window: far above W, caught at the next trip)
        }
        if (!out) return S5GPU_STATUS_PATH_ROW;
    }
    return S5GPU_STATUS_PATH_ROW;
}

#ifndef S5_DTW_HOST
struct LongQueryArgs {
    const s5gpu_event_t *rows;
    const uint64_t *first;           // n + 1
    const int32_t *ev_status;        // may be nullptr: every read 0
    uint64_t total_rows;
    uint32_t skip, emin, emax;
    double scale;
    int32_t clip;
    int16_t *queries;                // [total_rows]
    uint32_t *qlen;
    int32_t *status;
};
struct BandArgs {
    const int16_t *queries;          // [total_rows], read i at first[i]
    const uint64_t *first;           // n + 1
    const uint32_t *qlen;
    uint64_t total_rows;
    const int16_t *ref;
    uint32_t R;
    const int32_t *anchor;           // read i: anchor[i * anchor_stride]
    uint32_t anchor_stride;
    const int32_t *status_in;
    uint64_t row0;                   // first[0] of this launch's reads: their slots are counted from it
    uint32_t T, band;
    uint32_t *scratch;               // `slots` slots of slot_words * 64 words
    int32_t *tile_a;                 // [slots], behind them
    uint64_t slots;
    uint32_t slot_words;
    s5gpu_ext_row_t *rows_out;
    int32_t *lo, *hi;                // [total_rows]
};
// k_ev_query_long over n reads, on st
int launch_queries_long(uint32_t n, const LongQueryArgs &A, hipStream_t st);
// k_sdtw_band<T / 64> and k_sdtw_band_trace over n reads, on st
int launch_band(uint32_t n, const BandArgs &A, hipStream_t st);
// s5gpu_set_option's key of the band call
int set_option(const char *key, long value);
#endif

}  // namespace bandk
