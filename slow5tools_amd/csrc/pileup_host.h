// pileup_host.h — host code that pileup_api.hip, contrast_api.hip and sites_api.hip share (docs/codecs.md §4.22, §4.23, §4.25): the checks of
// a ragged call, and the batch of a whole-read handle, which feeds a table, a histogram, the site matrix or any of them from one run of
// extend's chain.
#pragma once
#include "refine_host.h"
#include "sites_dev.h"

namespace pilek {

// The argument checks of s5gpu_pileup_accum_long_dev and s5gpu_pile_hist_accum_long_dev (who names the caller), then launch_pileup_long.
// A.acc with A.ref: the table, or NULL; hist: the histogram, or NULL; the one who's call is about must be there.
int accum_long_checked(const char *who, const PileLongArgs &A, size_t work_bytes, void *hist, bool hist_call, hipStream_t st);
// The checks every ragged call makes of its layout and its work area (the tail of the above).  *go: there is something to launch (n > 0).
int long_layout_check(const char *who, const PileLongArgs &A, size_t work_bytes, bool *go);

// The whole-read chain of one handle
struct WholeChain {
    s5gpu_event_params_t ep;
    s5gpu_map_params_t mp;
    s5gpu_band_params_t bp;
    size_t scratch_max = 0;
    std::vector<int16_t> ref;
    bool refine = false;                                                   // §4.24: the rounds behind each group's band call; the table and the histogram
    s5gpu_refine_params_t rp;                                              // are fed with the refined queries, paths and statuses
    bool started = false;                                                  // a batch has been added: the parameters stay as they are
};
// s5gpu_pileup_set_refine and s5gpu_contrast_set_refine on the chain of a whole-read handle
int whole_set_refine(const char *who, WholeChain &W, const s5gpu_refine_params_t *rp);
// the checks of s5gpu_pileup_open_whole, but for the device's: a message and S5GPU_ERR_ARG
int whole_open_check(const char *who, const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, const int16_t *ref_host, uint32_t R);
// What a batch leaves of the sites of §4.25: the cells of its n records at the M columns d_sites lists, [M][n] on the host, and where
// scores_out is given their rows against d_control.  A record that never reached the device has empty entries.
struct SiteSink {
    const uint32_t *d_sites;
    uint32_t M;
    const void *d_control;
    s5gpu_site_cell_t *cells_out;
    s5gpu_site_score_t *scores_out;
};
// The two halves of a sink (sites_api.hip), on the front's stream, which both wait for.  _reads: the m reads of the front, whose ragged batch
// is A, at their records' places of the sink's arrays; _rest: the entries of the records that never reached the device.
int site_sink_reads(const PileLongArgs &A, size_t work_bytes, const SiteSink &S, const dtwk::MapFront &F, uint32_t n, hipStream_t st);
int site_sink_rest(const SiteSink &S, const dtwk::MapFront &F, uint32_t n, uint32_t R, hipStream_t st);
// s5gpu_pileup_add_batch_whole on the chain W into whichever of d_acc, d_hist and sites is given
int add_batch_whole(const char *who, const WholeChain &W, void *d_acc, void *d_hist, const SiteSink *sites, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method,
                    int sig_method, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out);

}  // namespace pilek
