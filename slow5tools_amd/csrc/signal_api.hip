// signal_api.hip — host side of the signal calls (include/slow5gpu.h, "signals"): argument checks and launches of the two device entry
// points, and s5gpu_signal_stats_stream: upload of a file chunk -> decode (fields + signals only where the methods allow it) -> k_sig_stats
// -> one small download.  The decoded signals never leave the device.
#include "host_ctx.h"
#include "signal_dev.h"

namespace {

int check_common(const char *who, uint32_t n, const void *sig, const void *sig_off, const void *sig_cap, const void *fields) {
    if (n && (!sig || !sig_off || !sig_cap || !fields)) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)sig & 15u) || ((uintptr_t)sig_off & 7u) || ((uintptr_t)sig_cap & 3u) || ((uintptr_t)fields & 7u)) {
        s5gpu_set_error("%s: misaligned argument (sig: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    return S5GPU_OK;
}

int check_quantiles(const char *who, uint32_t n_q, const double *q, sigk::Quantiles *Q) {
    if (n_q > 4) { s5gpu_set_error("%s: %u quantiles (at most 4)", who, n_q); return S5GPU_ERR_ARG; }
    if (n_q && !q) { s5gpu_set_error("%s: NULL quantiles", who); return S5GPU_ERR_ARG; }
    memset(Q, 0, sizeof *Q);
    Q->n = n_q;
    for (uint32_t k = 0; k < n_q; k++) {
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) { s5gpu_set_error("%s: quantile %u = %g lies outside [0, 1]", who, k, q[k]); return S5GPU_ERR_ARG; }
        Q->q[k] = q[k];
    }
    return S5GPU_OK;
}

}  // namespace

extern "C" int s5gpu_signal_stats_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                                      uint32_t n_q, const double *q, s5gpu_sig_stats_t *stats, void *stream) {
    sigk::Quantiles Q;
    int rc;
    if ((rc = check_quantiles("s5gpu_signal_stats_dev", n_q, q, &Q)) || (rc = check_common("s5gpu_signal_stats_dev", n, sig, sig_off, sig_cap, fields))) return rc;
    if (n && (!stats || ((uintptr_t)stats & 7u))) { s5gpu_set_error("s5gpu_signal_stats_dev: NULL or misaligned stats"); return S5GPU_ERR_ARG; }
    const sigk::SigRecs R = {sig, (const uint8_t *)sig_off, (const uint8_t *)sig_cap, fields, sizeof(uint64_t), sizeof(uint32_t), n};
    return sigk::launch_stats(R, Q, stats, (hipStream_t)stream);
}

extern "C" int s5gpu_signal_windows_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                                        const s5gpu_sig_stats_t *stats, uint32_t n_windows, const uint32_t *win_read, const uint32_t *win_start, uint32_t W,
                                        int mode, double a, double b, int dtype, void *out, int32_t *win_status, void *stream) {
    const char *who = "s5gpu_signal_windows_dev";
    if (W == 0) { s5gpu_set_error("%s: W = 0", who); return S5GPU_ERR_ARG; }
    if (mode != S5GPU_NORM_RAW && mode != S5GPU_NORM_PA && mode != S5GPU_NORM_MEDMAD && mode != S5GPU_NORM_QUANT) {
        s5gpu_set_error("%s: unknown mode %d", who, mode);
        return S5GPU_ERR_ARG;
    }
    if (dtype != S5GPU_SIG_F32 && dtype != S5GPU_SIG_F16) { s5gpu_set_error("%s: unknown dtype %d", who, dtype); return S5GPU_ERR_ARG; }
    if (n_windows == 0) return S5GPU_OK;
    int rc;
    if ((rc = check_common(who, n, sig, sig_off, sig_cap, fields))) return rc;
    if (!win_read || !win_start || !out || !win_status) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if ((uintptr_t)out & 15u) { s5gpu_set_error("%s: out is not 16-byte aligned", who); return S5GPU_ERR_ARG; }
    if ((mode == S5GPU_NORM_MEDMAD || mode == S5GPU_NORM_QUANT) && n && !stats) { s5gpu_set_error("%s: this mode needs stats", who); return S5GPU_ERR_ARG; }
    const sigk::SigRecs R = {sig, (const uint8_t *)sig_off, (const uint8_t *)sig_cap, fields, sizeof(uint64_t), sizeof(uint32_t), n};
    sigk::WinArgs A;
    A.stats = stats; A.win_read = win_read; A.win_start = win_start; A.win_status = win_status; A.out = out;
    A.n_windows = n_windows; A.W = W; A.mode = mode; A.a = a; A.b = b;
    return sigk::launch_windows(R, A, dtype, (hipStream_t)stream);
}

extern "C" int s5gpu_signal_stats_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                                         int sig_method, uint32_t n_q, const double *q, s5gpu_sig_stats_t *stats_out, s5gpu_rec_fields_t *fields_out) {
    const char *who = "s5gpu_signal_stats_stream";
    sigk::Quantiles Q;
    int rc;
    if ((rc = check_quantiles(who, n_q, q, &Q))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len || !stats_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    uint64_t b0, e1;
    if ((rc = s5rules::chunk_span(who, "record", n, chunk_bytes, rec_pos, rec_len, &b0, &e1))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    std::vector<s5gpu_rec_fields_t> ff;
    int drc;
    if (s5rules::decodes_without_payload(rec_method, sig_method)) {
        if ((rc = c->d_in.reserve(e1 - b0 + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_in.p, (const uint8_t *)chunk + b0, e1 - b0, hipMemcpyHostToDevice, c->st));
        drc = s5host::decode_np_framed(c, who, n, (const uint8_t *)chunk, b0, rec_pos, rec_len, rec_method, sig_method, ff);
    } else {
        std::vector<const void *> rec(n);
        std::vector<size_t> len(n);
        std::vector<s5gpu_rec_desc_t> rd;
        for (uint32_t i = 0; i < n; i++) { rec[i] = (const uint8_t *)chunk + rec_pos[i]; len[i] = rec_len[i]; }
        drc = s5host::decode_resident_framed(c, n, rec.data(), len.data(), rec_method, sig_method, rd, ff, nullptr, (const uint8_t *)chunk + b0, (size_t)(e1 - b0));
    }
    if (drc && drc != S5GPU_ERR_DATA) return drc;
    // the statistics of what the decode left on the device: a failed record has n_eff = 0, so the kernel reads nothing of it
    if ((rc = c->d_patch.reserve(sizeof(s5gpu_sig_stats_t) * n)) || (rc = c->h_out.reserve(sizeof(s5gpu_sig_stats_t) * (size_t)n + 64))) return rc;
    if ((rc = sigk::launch_stats(s5host::resident_sig_recs(c, n), Q, (s5gpu_sig_stats_t *)c->d_patch.p, c->st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_patch.p, sizeof(s5gpu_sig_stats_t) * n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(stats_out, c->h_out.p, sizeof(s5gpu_sig_stats_t) * n);
    if (fields_out) memcpy(fields_out, ff.data(), sizeof(s5gpu_rec_fields_t) * n);
    if (drc) s5gpu_set_error("%s: at least one record is corrupt (see stats_out[i].status)", who);
    return drc;
}
