// dtw_host.h — what the host sides of map, align and pileup (dtw_api.hip, dtw_path_api.hip, pileup_api.hip) share: the front of the batch
// chain, the path tail behind it, and the way results go back to the caller's records.
#pragma once
#include "dtw_dev.h"
#include "host_ctx.h"

namespace dtwk {

constexpr size_t SCRATCH_MAX = (size_t)256 << 20;                          // the scratch of a batch call's paths at most
constexpr s5gpu_map_row_t EMPTY_ROW = {NO_COST, 0, -1, -1};                // the row of a read without a query, and of a record that was dropped

int check_ref(const char *who, uint32_t R);                                // 1 .. 2^31 - 1 reference values
int check_wmax(const char *who, uint32_t wmax);                            // 1 .. WMAX columns

// What map_front leaves behind: the context it holds (its stream has the work queued) and, on that context's device, the event rows of the
// m records that decoded (the front's Resident), their prefix, the query matrix [m, qmax], qlen[m], the reference, and room for m result rows
// (in c->d_patch and c->d_stream, which the caller must not reserve again).
struct MapFront : s5host::Resident {
    s5host::CtxHold hold;
    const s5gpu_event_t *d_rows = nullptr;
    const uint64_t *d_first = nullptr;
    int16_t *d_q = nullptr;
    uint32_t *d_ql = nullptr;
    int16_t *d_ref = nullptr;
    s5gpu_map_row_t *d_out = nullptr;
    const int32_t *d_est = nullptr;                                        // the events' statuses [m]
    uint64_t total = 0;                                                    // the event rows of the m reads: first[m], which the host knows
};
// the S5GPU_ERR_ARG cases of s5gpu_map_batch, before a device is needed; outputs: the caller's own output pointers are there
int map_front_check(const char *who, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                    const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, bool outputs);
// upload -> decode (again without the corrupt records where others still wait for a larger slot) -> event count pass, scan, fill pass ->
// queries, for n >= 1 checked records on the first device in use
int map_front(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
              const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, MapFront &F);

// The path tail behind a front with m >= 1 reads: sDTW with the start -> the paths -> (events) the query's event rows gathered, queued on the
// front's stream.  Everything lands in one block of c->d_gather, at the offsets of path_layout: the rows [m] at 0, the path statuses [m], lo
// and hi [m, qmax], the events [m, qmax]; `bytes` of it in all, the first o_lo of which are the rows and statuses.  Uses c->d_scan as
// scratch, and reserves c->h_out for the `back` bytes the caller will bring back.
struct PathTail { size_t o_pst, o_lo, o_hi, o_ev, bytes; };
PathTail path_layout(uint32_t m, uint32_t qmax, bool events);
int path_scratch_check(const char *who, uint32_t qmax, uint32_t wmax);      // S5GPU_ERR_NOMEM: one read's scratch is above SCRATCH_MAX
int path_tail(const MapFront &F, const s5gpu_map_params_t *mp, uint32_t wmax, uint32_t R, bool events, const PathTail &T, size_t back);
// The rows hr[m] (and the path statuses h_pst[m], NULL: there were no paths) of the front's reads, put at their records' places: rows_out[n]
// (NULL: not wanted) is EMPTY_ROW elsewhere; a decoded read's status becomes QUERY_SHORT where it has no query, else its path status.
void scatter_rows(MapFront &F, uint32_t n, const s5gpu_map_row_t *hr, const int32_t *h_pst, s5gpu_map_row_t *rows_out);

}  // namespace dtwk
