// dtw_path_api.hip — host side of the align calls (include/slow5gpu.h, "align"; docs/codecs.md §4.17): the slot size, argument checks and
// the grouped launches of s5gpu_sdtw_path_dev, and s5gpu_align_batch: the front of s5gpu_map_batch (dtw_host.h) -> sDTW with the start ->
// the paths -> the query's event rows gathered -> one download of rows, statuses, lo, hi and events.
#include "dtw_host.h"

namespace {

uint32_t g_passes = 3;                                                     // option "sdtw_path_passes"

bool path_shape_ok(uint32_t qpitch, uint32_t wmax) { return qpitch >= 1 && qpitch <= dtwk::QMAX && wmax >= 1 && wmax <= dtwk::WMAX; }

}  // namespace

int dtwk::path_set_option(const char *key, long value) {
    // which passes s5gpu_sdtw_path_dev launches: 1 k_sdtw_dirs only, 2 k_sdtw_trace only (over what an earlier call left in the scratch),
    // 3 both (the default).  For tools/sdtw_path_time.py: the passes are timed apart.
    if (key && strcmp(key, "sdtw_path_passes") == 0 && value >= 1 && value <= 3) { g_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

extern "C" size_t s5gpu_sdtw_path_slot_bytes(uint32_t qpitch, uint32_t wmax) {
    if (!path_shape_ok(qpitch, wmax)) return 0;
    return (size_t)dtwk::path_slot_words(qpitch, wmax) * 256u;
}

extern "C" int s5gpu_sdtw_path_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                                   const s5gpu_map_row_t *rows, uint32_t wmax, void *scratch, size_t scratch_bytes, int32_t *lo, int32_t *hi,
                                   int32_t *status, void *stream) {
    const char *who = "s5gpu_sdtw_path_dev";
    if (qpitch == 0 || qpitch > dtwk::QMAX) { s5gpu_set_error("%s: a pitch of %u values (1 .. %u)", who, qpitch, dtwk::QMAX); return S5GPU_ERR_ARG; }
    int rc;
    if ((rc = dtwk::check_ref(who, R)) || (rc = dtwk::check_wmax(who, wmax))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !rows || !scratch || !lo || !hi || !status) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)queries & 1u) || ((uintptr_t)qlen & 3u) || ((uintptr_t)ref & 1u) || ((uintptr_t)rows & 15u) || ((uintptr_t)scratch & 15u) ||
        ((uintptr_t)lo & 3u) || ((uintptr_t)hi & 3u) || ((uintptr_t)status & 3u)) {
        s5gpu_set_error("%s: misaligned argument (rows, scratch: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    const size_t slot = s5gpu_sdtw_path_slot_bytes(qpitch, wmax);
    if (scratch_bytes < slot) { s5gpu_set_error("%s: a scratch of %zu bytes, a read needs %zu", who, scratch_bytes, slot); return S5GPU_ERR_NOMEM; }
    const size_t fit = scratch_bytes / slot;
    const uint32_t group = fit < n ? (uint32_t)fit : n;
    // a group of reads at a time, each in the slot of its place in the group; the stream orders the groups, so the scratch is used again
    for (uint32_t b = 0; b < n; b += group) {
        dtwk::PathArgs A;
        A.queries = queries + (size_t)b * qpitch; A.qpitch = qpitch; A.qlen = qlen + b; A.ref = ref; A.R = R;
        A.rows = reinterpret_cast<const dtwk::U4 *>(rows) + b; A.wmax = wmax;
        A.scratch = (uint32_t *)scratch; A.slot_words = dtwk::path_slot_words(qpitch, wmax);
        A.lo = lo + (size_t)b * qpitch; A.hi = hi + (size_t)b * qpitch; A.status = status + b;
        if ((rc = dtwk::launch_path(n - b < group ? n - b : group, A, (hipStream_t)stream, (int)g_passes))) return rc;
    }
    return S5GPU_OK;
}

int dtwk::check_wmax(const char *who, uint32_t wmax) {
    if (wmax == 0 || wmax > WMAX) { s5gpu_set_error("%s: wmax %u (1 .. %u)", who, wmax, WMAX); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

int dtwk::path_scratch_check(const char *who, uint32_t qmax, uint32_t wmax) {
    const size_t slot = s5gpu_sdtw_path_slot_bytes(qmax, wmax);
    if (slot > SCRATCH_MAX) { s5gpu_set_error("%s: a read needs %zu bytes of scratch, above the %zu of this call", who, slot, SCRATCH_MAX); return S5GPU_ERR_NOMEM; }
    return S5GPU_OK;
}

dtwk::PathTail dtwk::path_layout(uint32_t m, uint32_t qmax, bool events) {
    PathTail T;
    T.o_pst = up(16ull * m, 16); T.o_lo = T.o_pst + up(4ull * m, 16); T.o_hi = T.o_lo + up(4ull * m * qmax, 16);
    T.o_ev = T.o_hi + up(4ull * m * qmax, 16); T.bytes = T.o_ev + (events ? 16ull * m * qmax : 0);
    return T;
}

int dtwk::path_tail(const MapFront &F, const s5gpu_map_params_t *mp, uint32_t wmax, uint32_t R, bool events, const PathTail &T, size_t back) {
    Ctx *c = F.hold.c;
    const uint32_t m = F.m, qmax = mp->qmax;
    const size_t slot = s5gpu_sdtw_path_slot_bytes(qmax, wmax), scratch = slot * m < SCRATCH_MAX ? slot * m : SCRATCH_MAX / slot * slot;
    int rc;
    if ((rc = c->d_gather.reserve(T.bytes + 64)) || (rc = c->d_scan.reserve(scratch + 64)) || (rc = c->h_out.reserve(back + 64))) return rc;
    uint8_t *dg = (uint8_t *)c->d_gather.p;
    s5gpu_map_row_t *d_out = (s5gpu_map_row_t *)dg;
    if ((rc = launch_sdtw(m, F.d_q, qmax, F.d_ql, F.d_ref, R, true, d_out, c->st)) ||
        (rc = s5gpu_sdtw_path_dev(m, F.d_q, qmax, F.d_ql, F.d_ref, R, d_out, wmax, c->d_scan.p, scratch, (int32_t *)(dg + T.o_lo), (int32_t *)(dg + T.o_hi),
                                  (int32_t *)(dg + T.o_pst), c->st)))
        return rc;
    return events ? launch_event_gather(m, F.d_rows, F.d_first, F.d_ql, mp->skip, qmax, (s5gpu_event_t *)(dg + T.o_ev), c->st) : S5GPU_OK;
}

void dtwk::scatter_rows(MapFront &F, uint32_t n, const s5gpu_map_row_t *hr, const int32_t *h_pst, s5gpu_map_row_t *rows_out) {
    if (rows_out)
        for (uint32_t i = 0; i < n; i++) rows_out[i] = EMPTY_ROW;
    for (uint32_t k = 0; k < F.m; k++) {
        const uint32_t i = F.cur[k];
        if (rows_out) rows_out[i] = hr[k];
        if (F.status[i] == 0) F.status[i] = hr[k].qlen == 0 ? S5GPU_STATUS_QUERY_SHORT : h_pst ? h_pst[k] : 0;
    }
}

extern "C" int s5gpu_align_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                 const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, uint32_t wmax, const int16_t *ref_host, uint32_t R,
                                 s5gpu_map_row_t *rows_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out, int32_t *status_out) {
    const char *who = "s5gpu_align_batch";
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, rows_out && lo_out && hi_out))) return rc;
    if ((rc = dtwk::check_wmax(who, wmax))) return rc;
    if (n == 0) return S5GPU_OK;
    if ((rc = dtwk::path_scratch_check(who, mp->qmax, wmax))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, F))) return rc;
    Ctx *c = F.hold.c;
    const size_t row_i = (size_t)mp->qmax;
    for (size_t x = 0; x < (size_t)n * row_i; x++) { lo_out[x] = -1; hi_out[x] = -1; }  // what a record that was dropped keeps
    if (events_out) memset(events_out, 0, sizeof(s5gpu_event_t) * (size_t)n * row_i);
    const dtwk::PathTail T = dtwk::path_layout(F.m, mp->qmax, events_out != nullptr);
    if (F.m) {
        if ((rc = dtwk::path_tail(F, mp, wmax, R, events_out != nullptr, T, T.bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_gather.p, T.bytes, hipMemcpyDeviceToHost, c->st));   // rows, statuses, lo, hi and events at once
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    const uint8_t *h = (const uint8_t *)c->h_out.p;
    dtwk::scatter_rows(F, n, (const s5gpu_map_row_t *)h, (const int32_t *)(h + T.o_pst), rows_out);
    for (uint32_t k = 0; k < F.m; k++) {
        const size_t i = F.cur[k];
        memcpy(lo_out + i * row_i, h + T.o_lo + 4 * k * row_i, 4 * row_i);
        memcpy(hi_out + i * row_i, h + T.o_hi + 4 * k * row_i, 4 * row_i);
        if (events_out) memcpy(events_out + i * row_i, h + T.o_ev + 16 * k * row_i, 16 * row_i);
    }
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its outputs are empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
