// pileup_host.h — host code that pileup_api.hip and contrast_api.hip share (docs/codecs.md §4.22, §4.23): the checks of a ragged call, and
// the batch of a whole-read handle, which feeds a table, a histogram or both from one run of extend's chain.
#pragma once
#include "refine_host.h"
#include "pileup_dev.h"

namespace pilek {

// The argument checks of s5gpu_pileup_accum_long_dev and s5gpu_pile_hist_accum_long_dev (who names the caller), then launch_pileup_long.
// A.acc with A.ref: the table, or NULL; hist: the histogram, or NULL; the one who's call is about must be there.
int accum_long_checked(const char *who, const PileLongArgs &A, size_t work_bytes, void *hist, bool hist_call, hipStream_t st);

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
// s5gpu_pileup_add_batch_whole on the chain W into d_acc and, when given, d_hist
int add_batch_whole(const char *who, const WholeChain &W, void *d_acc, void *d_hist, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method,
                    int sig_method, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out);

}  // namespace pilek
