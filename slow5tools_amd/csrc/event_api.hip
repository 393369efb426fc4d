// event_api.hip — host side of the event calls (include/slow5gpu.h, "events"): argument checks and the launch of the device entry point, and
// s5gpu_signal_events_batch: upload -> decode -> count pass -> exclusive scan -> fill pass -> the rows come back.  The decoded signals never
// leave the device.
#include <math.h>

#include "event_dev.h"
#include "host_ctx.h"

namespace {

int check_params(const char *who, const s5gpu_event_params_t *p, int mode) {
    if (!p) { s5gpu_set_error("%s: NULL parameters", who); return S5GPU_ERR_ARG; }
    if (p->w1 == 0 || p->w1 >= p->w2 || p->w2 > 64) { s5gpu_set_error("%s: windows %u, %u (1 <= w1 < w2 <= 64)", who, p->w1, p->w2); return S5GPU_ERR_ARG; }
    if (!isfinite(p->thr1) || !isfinite(p->thr2) || !isfinite(p->peak_height)) { s5gpu_set_error("%s: a threshold is not finite", who); return S5GPU_ERR_ARG; }
    if (mode != S5GPU_NORM_RAW && mode != S5GPU_NORM_PA) { s5gpu_set_error("%s: mode %d (raw or pA)", who, mode); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

evk::EvArgs args_of(const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows, uint32_t *n_events,
                    int32_t *ev_status) {
    evk::EvArgs A;
    A.w1 = p->w1; A.w2 = p->w2; A.thr1 = p->thr1; A.thr2 = p->thr2; A.peak_height = p->peak_height; A.mode = mode;
    A.ev_off = ev_off; A.ev_cap = ev_cap; A.rows = rows; A.n_events = n_events; A.ev_status = ev_status;
    return A;
}

}  // namespace

extern "C" int s5gpu_signal_events_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                                       const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows,
                                       uint32_t *n_events, int32_t *ev_status, void *stream) {
    const char *who = "s5gpu_signal_events_dev";
    int rc;
    if ((rc = check_params(who, p, mode))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!sig || !sig_off || !sig_cap || !fields || !n_events || !ev_status || (rows && (!ev_off || !ev_cap))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)sig & 15u) || ((uintptr_t)sig_off & 7u) || ((uintptr_t)sig_cap & 3u) || ((uintptr_t)fields & 7u) || ((uintptr_t)rows & 15u) ||
        ((uintptr_t)ev_off & 7u) || ((uintptr_t)ev_cap & 3u) || ((uintptr_t)n_events & 3u) || ((uintptr_t)ev_status & 3u)) {
        s5gpu_set_error("%s: misaligned argument (sig, rows: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    const sigk::SigRecs R = {sig, (const uint8_t *)sig_off, (const uint8_t *)sig_cap, fields, sizeof(uint64_t), sizeof(uint32_t), n};
    return evk::launch_events(R, args_of(p, mode, ev_off, ev_cap, rows, n_events, ev_status), (hipStream_t)stream);
}

extern "C" int s5gpu_signal_events_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                         const s5gpu_event_params_t *p, int mode, s5gpu_event_t *rows_out, size_t rows_cap, uint64_t *ev_first,
                                         int32_t *status_out) {
    const char *who = "s5gpu_signal_events_batch";
    int rc;
    if ((rc = check_params(who, p, mode))) return rc;
    if ((rec_method != S5GPU_REC_NONE && rec_method != S5GPU_REC_ZLIB && rec_method != S5GPU_REC_ZSTD) ||
        (sig_method != S5GPU_SIG_NONE && sig_method != S5GPU_SIG_SVB_ZD && sig_method != S5GPU_SIG_EX_ZD)) {
        s5gpu_set_error("%s: unsupported method", who);
        return S5GPU_ERR_ARG;
    }
    if (!ev_first || (n && (!rec || !rec_len)) || (rows_cap && !rows_out)) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    for (uint32_t i = 0; i < n; i++)
        if (!rec[i] && rec_len[i]) { s5gpu_set_error("%s: record %u is NULL", who, i); return S5GPU_ERR_ARG; }
    if (n == 0) { ev_first[0] = 0; return S5GPU_OK; }
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    // the decode; a batch with corrupt records is decoded again without them while others still wait for a larger slot (host_ctx.h)
    std::vector<s5gpu_rec_desc_t> rd;
    std::vector<s5gpu_rec_fields_t> ff;
    std::vector<uint32_t> cur;
    std::vector<int32_t> status(n, 0);
    std::vector<const void *> r2;
    std::vector<size_t> l2;
    bool corrupt = false;
    auto decode = [&](uint32_t m, const uint32_t *idx) {
        r2.resize(m); l2.resize(m);
        for (uint32_t k = 0; k < m; k++) { r2[k] = rec[idx[k]]; l2[k] = rec_len[idx[k]]; }
        return s5host::decode_resident(c, m, r2.data(), l2.data(), rec_method, sig_method, rd, ff, nullptr);
    };
    if ((rc = s5host::decode_dropping_corrupt(n, decode, ff, cur, status.data(), &corrupt))) return rc;
    if (status_out) memcpy(status_out, status.data(), sizeof(int32_t) * n);
    const uint32_t m = (uint32_t)cur.size();
    // on the device: first[m + 1] (u64), then cnt[m] (u32) and the kernel's statuses [m]
    const size_t o_cnt = up(8ull * (m + 1), 16), o_st = o_cnt + up(4ull * m, 16);
    if ((rc = c->d_patch.reserve(o_st + 4ull * m + 64)) || (rc = c->h_out.reserve(8ull * (m + 1) + 64))) return rc;
    uint64_t *d_first = (uint64_t *)c->d_patch.p;
    uint32_t *d_cnt = (uint32_t *)((uint8_t *)c->d_patch.p + o_cnt);
    int32_t *d_st = (int32_t *)((uint8_t *)c->d_patch.p + o_st);
    const sigk::SigRecs R = {(const int16_t *)c->d_sig2.p, (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_off),
                             (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_cap), (const s5gpu_rec_fields_t *)c->d_fields.p,
                             sizeof(s5gpu_rec_desc_t), sizeof(s5gpu_rec_desc_t), m};
    if ((rc = evk::launch_events(R, args_of(p, mode, nullptr, nullptr, nullptr, d_cnt, d_st), c->st)) || (rc = evk::launch_scan(m, d_cnt, d_first, c->st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_out.p, d_first, 8ull * (m + 1), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    const uint64_t *first = (const uint64_t *)c->h_out.p;
    const uint64_t total = first[m];
    if (total > rows_cap) {
        ev_first[0] = total;
        s5gpu_set_error("%s: %llu rows needed, room for %zu", who, (unsigned long long)total, rows_cap);
        return S5GPU_ERR_NOMEM;
    }
    for (uint32_t i = 0, k = 0; i <= n; i++) {                            // a record that was dropped has no rows
        ev_first[i] = first[k];
        if (k < m && i == cur[k]) k++;
    }
    if (total) {
        if ((rc = c->d_stream.reserve(16ull * total + 64))) return rc;
        if ((rc = evk::launch_events(R, args_of(p, mode, d_first, d_cnt, (s5gpu_event_t *)c->d_stream.p, d_cnt, d_st), c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(rows_out, c->d_stream.p, 16ull * total, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    if (corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and it has no events)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
