// event_host.h — what the host side of events (event_api.hip) lends to the front of map, align and pileup (dtw_api.hip).
#pragma once
#include "event_dev.h"
#include "host_ctx.h"

namespace evk {

// the S5GPU_ERR_ARG cases of an event call's parameters
int check_params(const char *who, const s5gpu_event_params_t *p, int mode);
// the kernel's arguments: rows = NULL for the count pass; for the fill pass the scan's offsets, the counts as capacities and the rows
EvArgs args_of(const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows, uint32_t *n_events,
               int32_t *ev_status);
// The count pass of k_sig_events over the records S a decode left in the context c, and the scan, queued on c->st: counts in d_cnt[S.n],
// statuses in d_st[S.n], the prefix in d_first[S.n + 1]; then the last `back` entries of d_first (1: the total alone, S.n + 1: all of it)
// brought to c->h_out and waited for; *total = the rows the batch needs.  The fill pass is the caller's launch_events with
// args_of(p, mode, d_first, d_cnt, rows, d_cnt, d_st), once it has made room for the rows.
int events_count(Ctx *c, const sigk::SigRecs &S, const s5gpu_event_params_t *p, int mode, uint64_t *d_first, uint32_t *d_cnt, int32_t *d_st,
                 uint32_t back, uint64_t *total);

}  // namespace evk
