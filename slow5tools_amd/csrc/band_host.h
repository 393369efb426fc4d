// band_host.h — what the host sides of extend and of the whole-read pileup (band_api.hip, pileup_api.hip) share: the checks of the band
// parameters and the device side of s5gpu_extend_batch behind the front of dtw_host.h.
#pragma once
#include <vector>

#include "dtw_host.h"
#include "band_dev.h"

namespace bandk {

int check_band_params(const char *who, const s5gpu_band_params_t *p);      // every parameter inside its range (§4.21)
// skip, scale and clip of the band parameters are those of the map parameters
int check_band_agrees(const char *who, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp);

// What extend_tail leaves in one block of c->d_gather, for the m reads of a front: the result rows [m] at 0, the prefix rows [m] at o_map,
// lo and hi [total] at o_lo and o_hi and room for a copy of the event rows at o_ev (events), `back` bytes in all, which may come back in
// one copy; behind them the long queries [total] at o_q, their lengths [m] at o_ql and statuses [m] at o_st, which do not.  first: the
// prefix of the reads' event rows, on the host; too_big[k]: read k's scratch alone is above scratch_max and it was passed over (its result
// row was not written).
struct ExtTail {
    size_t o_map = 0, o_lo = 0, o_hi = 0, o_ev = 0, back = 0, o_q = 0, o_ql = 0, o_st = 0;
    // with the rounds of §4.24 (refine parameters given), behind all of that: the refined rows [m] at r_rows (= r_base), the fits [m] at
    // r_fit, the rounds [m] at r_rnd, the refined lo, hi and queries [total] at r_lo, r_hi and r_q, which may come back in one copy of
    // [r_base, r_back); behind them the work area of the rounds at r_work
    size_t r_base = 0, r_rows = 0, r_fit = 0, r_rnd = 0, r_lo = 0, r_hi = 0, r_q = 0, r_back = 0, r_work = 0;
    std::vector<uint64_t> first;
    std::vector<uint8_t> too_big;
};
// Behind a front with m >= 1 reads (mp->want_start on): sDTW of the prefix with the start -> the long queries of the resident event rows ->
// the banded alignment from `start` in groups of consecutive reads whose scratch is at most scratch_max (0: 1 GiB), queued on the front's
// stream; the stream is synchronised once, for `first`.  rows_cap: the rows the caller has room for: above it S5GPU_ERR_NOMEM and
// *room_out = the rows that suffice, nothing queued.  c->d_scan is the scratch, reserved for at least scan_min bytes; c->h_out is reserved
// for `back` bytes (paths_back) or for the two row arrays and m statuses.  rp (may be NULL: nothing more is launched): the rounds of
// s5gpu_extend_refine_dev follow each group's band call, on the group's reads and in the group's scratch; c->h_out is then reserved for
// r_back bytes (paths_back) or for the row arrays, m statuses and the refined rows behind them.
int extend_tail(const char *who, dtwk::MapFront &F, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, size_t scratch_max, uint32_t R, bool events,
                bool paths_back, size_t rows_cap, size_t scan_min, uint64_t *room_out, ExtTail &E, const s5gpu_refine_params_t *rp = nullptr);
// The result rows h[m] of the front's reads put at their records' places in rows_out[n] (row_none elsewhere, S5GPU_STATUS_PATH_WIDE for a
// read that was passed over); a read's status becomes its row's where that is not 0.
void scatter_ext_rows(dtwk::MapFront &F, uint32_t n, const ExtTail &E, const uint8_t *h, s5gpu_ext_row_t *rows_out);

}  // namespace bandk
