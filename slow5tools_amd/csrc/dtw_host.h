// dtw_host.h — what the host sides of map and align (dtw_api.hip, dtw_path_api.hip) share: the front of the batch chain.
#pragma once
#include "dtw_dev.h"
#include "host_ctx.h"

namespace dtwk {

// What map_front leaves behind: the context it holds (its stream has the work queued) and, on that context's device, the event rows of the
// m records that decoded, their prefix, the query matrix [m, qmax], qlen[m], the reference, and room for m result rows (in c->d_patch and
// c->d_stream, which the caller must not reserve again).  cur[k]: which record of the batch read k is; status[i], all n records: the
// decoder's.
struct MapFront {
    s5host::CtxHold hold;
    uint32_t m = 0;
    std::vector<uint32_t> cur;
    std::vector<int32_t> status;
    bool corrupt = false;
    const s5gpu_event_t *d_rows = nullptr;
    const uint64_t *d_first = nullptr;
    int16_t *d_q = nullptr;
    uint32_t *d_ql = nullptr;
    int16_t *d_ref = nullptr;
    s5gpu_map_row_t *d_out = nullptr;
};
// the S5GPU_ERR_ARG cases of s5gpu_map_batch, before a device is needed; outputs: the caller's own output pointers are there
int map_front_check(const char *who, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                    const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, bool outputs);
// upload -> decode (again without the corrupt records where others still wait for a larger slot) -> event count pass, scan, fill pass ->
// queries, for n >= 1 checked records on the first device in use
int map_front(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
              const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, MapFront &F);

}  // namespace dtwk
