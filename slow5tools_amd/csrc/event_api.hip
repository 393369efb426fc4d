// event_api.hip — host side of the event calls (include/slow5gpu.h, "events"): argument checks and the launch of the device entry point, and
// s5gpu_signal_events_batch: upload -> decode -> count pass -> exclusive scan -> fill pass -> the rows come back.  The decoded signals never
// leave the device.
#include <math.h>

#include "event_host.h"

int evk::check_params(const char *who, const s5gpu_event_params_t *p, int mode) {
    if (!p) { s5gpu_set_error("%s: NULL parameters", who); return S5GPU_ERR_ARG; }
    if (p->w1 == 0 || p->w1 >= p->w2 || p->w2 > 64) { s5gpu_set_error("%s: windows %u, %u (1 <= w1 < w2 <= 64)", who, p->w1, p->w2); return S5GPU_ERR_ARG; }
    if (!isfinite(p->thr1) || !isfinite(p->thr2) || !isfinite(p->peak_height)) { s5gpu_set_error("%s: a threshold is not finite", who); return S5GPU_ERR_ARG; }
    if (mode != S5GPU_NORM_RAW && mode != S5GPU_NORM_PA) { s5gpu_set_error("%s: mode %d (raw or pA)", who, mode); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

evk::EvArgs evk::args_of(const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows, uint32_t *n_events,
                    int32_t *ev_status) {
    evk::EvArgs A;
    A.w1 = p->w1; A.w2 = p->w2; A.thr1 = p->thr1; A.thr2 = p->thr2; A.peak_height = p->peak_height; A.mode = mode;
    A.ev_off = ev_off; A.ev_cap = ev_cap; A.rows = rows; A.n_events = n_events; A.ev_status = ev_status;
    return A;
}

int evk::events_count(Ctx *c, const sigk::SigRecs &S, const s5gpu_event_params_t *p, int mode, uint64_t *d_first, uint32_t *d_cnt, int32_t *d_st,
                      uint32_t back, uint64_t *total) {
    int rc;
    if ((rc = c->h_out.reserve(8ull * back + 64))) return rc;
    if ((rc = launch_events(S, args_of(p, mode, nullptr, nullptr, nullptr, d_cnt, d_st), c->st)) || (rc = launch_scan(S.n, d_cnt, d_first, c->st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_out.p, d_first + (S.n + 1 - back), 8ull * back, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(total, (const uint64_t *)c->h_out.p + (back - 1), 8);
    return S5GPU_OK;
}


extern "C" int s5gpu_signal_events_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                                       const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows,
                                       uint32_t *n_events, int32_t *ev_status, void *stream) {
    const char *who = "s5gpu_signal_events_dev";
    int rc;
    if ((rc = evk::check_params(who, p, mode))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!sig || !sig_off || !sig_cap || !fields || !n_events || !ev_status || (rows && (!ev_off || !ev_cap))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)sig & 15u) || ((uintptr_t)sig_off & 7u) || ((uintptr_t)sig_cap & 3u) || ((uintptr_t)fields & 7u) || ((uintptr_t)rows & 15u) ||
        ((uintptr_t)ev_off & 7u) || ((uintptr_t)ev_cap & 3u) || ((uintptr_t)n_events & 3u) || ((uintptr_t)ev_status & 3u)) {
        s5gpu_set_error("%s: misaligned argument (sig, rows: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    const sigk::SigRecs R = {sig, (const uint8_t *)sig_off, (const uint8_t *)sig_cap, fields, sizeof(uint64_t), sizeof(uint32_t), n};
    return evk::launch_events(R, evk::args_of(p, mode, ev_off, ev_cap, rows, n_events, ev_status), (hipStream_t)stream);
}

extern "C" int s5gpu_signal_events_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                         const s5gpu_event_params_t *p, int mode, s5gpu_event_t *rows_out, size_t rows_cap, uint64_t *ev_first,
                                         int32_t *status_out) {
    const char *who = "s5gpu_signal_events_batch";
    int rc;
    if ((rc = evk::check_params(who, p, mode))) return rc;
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (!ev_first || (n && (!rec || !rec_len)) || (rows_cap && !rows_out)) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if ((rc = s5rules::host_records_ok(who, n, rec, rec_len))) return rc;
    if (n == 0) { ev_first[0] = 0; return S5GPU_OK; }
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    s5host::Resident R;
    if ((rc = s5host::resident_records(c, n, rec, rec_len, rec_method, sig_method, R))) return rc;
    if (status_out) memcpy(status_out, R.status, sizeof(int32_t) * n);
    const uint32_t m = R.m;
    // on the device: first[m + 1] (u64), then cnt[m] (u32) and the kernel's statuses [m]
    const size_t o_cnt = up(8ull * (m + 1), 16), o_st = o_cnt + up(4ull * m, 16);
    if ((rc = c->d_patch.reserve(o_st + 4ull * m + 64))) return rc;
    uint64_t *d_first = (uint64_t *)c->d_patch.p;
    uint32_t *d_cnt = (uint32_t *)((uint8_t *)c->d_patch.p + o_cnt);
    int32_t *d_st = (int32_t *)((uint8_t *)c->d_patch.p + o_st);
    const sigk::SigRecs S = s5host::resident_sig_recs(c, m);
    uint64_t total = 0;
    if ((rc = evk::events_count(c, S, p, mode, d_first, d_cnt, d_st, m + 1, &total))) return rc;
    const uint64_t *first = (const uint64_t *)c->h_out.p;
    if (total > rows_cap) {
        ev_first[0] = total;
        s5gpu_set_error("%s: %llu rows needed, room for %zu", who, (unsigned long long)total, rows_cap);
        return S5GPU_ERR_NOMEM;
    }
    for (uint32_t i = 0, k = 0; i <= n; i++) {                            // a record that was dropped has no rows
        ev_first[i] = first[k];
        if (k < m && i == R.cur[k]) k++;
    }
    if (total) {
        if ((rc = c->d_stream.reserve(16ull * total + 64))) return rc;
        if ((rc = evk::launch_events(S, evk::args_of(p, mode, d_first, d_cnt, (s5gpu_event_t *)c->d_stream.p, d_cnt, d_st), c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(rows_out, c->d_stream.p, 16ull * total, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    if (R.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and it has no events)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
