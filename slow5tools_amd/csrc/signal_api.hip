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

// fields + signals only (S5GPU_DEC_NO_PAYLOAD) of the framed records already uploaded to c->d_in: descriptors in c->d_desc2, signals in c->d_sig2,
// fields in c->d_fields and ff.  A record that outgrew its guessed scratch or signal slot (status 5 / 6) has the batch decoded again with the sizes
// it reported.  Corrupt records: S5GPU_ERR_DATA, everything else of the batch is in place.
int s5host::decode_np_framed(Ctx *c, uint32_t n, const uint8_t *chunk, uint64_t b0, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                             int sig_method, std::vector<s5gpu_rec_fields_t> &ff) {
    int rc;
    std::vector<uint32_t> pcap(n), scap(n);
    std::vector<s5gpu_rec_desc_t> rd(n);
    uint32_t max_in = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec_len[i] > 0xFFFFFF00u / 8) { s5gpu_set_error("record %u too large", i); return S5GPU_ERR_ARG; }
        const uint64_t g = s5host::payload_guess_of(rec_method, chunk + rec_pos[i], rec_len[i]);
        pcap[i] = (uint32_t)(g > 0xFFFFFF00ull ? 0xFFFFFF00ull : g);
        scap[i] = pcap[i];                       // a sample takes at least one payload byte in either signal format
        max_in = max_in > rec_len[i] ? max_in : rec_len[i];
    }
    ff.resize(n);
    if ((rc = c->d_desc2.reserve(sizeof(s5gpu_rec_desc_t) * n)) || (rc = c->d_fields.reserve(sizeof(s5gpu_rec_fields_t) * n)) ||
        (rc = c->h_in.reserve(sizeof(s5gpu_rec_desc_t) * n + 64)) || (rc = c->h_out.reserve(sizeof(s5gpu_rec_fields_t) * n + 64)))
        return rc;
    for (int attempt = 0;; attempt++) {
        uint64_t so = 0;
        uint32_t max_cap = 64;
        for (uint32_t i = 0; i < n; i++) {
            s5gpu_rec_desc_t &d = rd[i];
            memset(&d, 0, sizeof d);
            d.in_off = rec_pos[i] - b0; d.in_len = rec_len[i];
            d.sig_off = so; d.sig_cap = scap[i];
            so += up((uint64_t)scap[i] + 8, 8);
            max_cap = max_cap > pcap[i] ? max_cap : pcap[i];
        }
        // scratch: a slot per workgroup the decoder can use; more slots than records (and its fallback's) buy nothing
        const uint64_t slot = ((uint64_t)max_cap + 16 + 15) & ~15ull;
        uint64_t scratch = s5gpu_decode_scratch_bytes(max_cap);
        const uint64_t enough = 64 + slot * ((uint64_t)n + 257), floor_ = 64 + 2 * slot, ceil_ = 1ull << 30;
        if (scratch > enough) scratch = enough;
        if (scratch > ceil_) scratch = ceil_;
        if (scratch < floor_) scratch = floor_;
        if ((rc = c->d_pay.reserve(scratch)) || (rc = c->d_sig2.reserve(so * 2 + 64))) return rc;
        memcpy(c->h_in.p, rd.data(), sizeof(s5gpu_rec_desc_t) * n);
        HIP_TRY(hipMemcpyAsync(c->d_desc2.p, c->h_in.p, sizeof(s5gpu_rec_desc_t) * n, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemsetAsync(c->d_fields.p, 0, sizeof(s5gpu_rec_fields_t) * n, c->st));
        s5gpu_decode_args_t da;
        memset(&da, 0, sizeof da);
        da.n_recs = n; da.rec_method = rec_method; da.sig_method = sig_method; da.flags = S5GPU_DEC_NO_PAYLOAD;
        da.desc = (const s5gpu_rec_desc_t *)c->d_desc2.p; da.in = (const uint8_t *)c->d_in.p;
        da.payload = (uint8_t *)c->d_pay.p; da.payload_bytes = scratch; da.max_pay_cap = max_cap; da.max_in_len = max_in;
        da.sig_out = (int16_t *)c->d_sig2.p; da.fields = (s5gpu_rec_fields_t *)c->d_fields.p;
        if ((rc = s5gpu_decode_dev(&da, c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_fields.p, sizeof(s5gpu_rec_fields_t) * n, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        memcpy(ff.data(), c->h_out.p, sizeof(s5gpu_rec_fields_t) * n);
        bool retry = false, bad = false;
        for (uint32_t i = 0; i < n; i++) {
            if (ff[i].status == 5 && attempt < 2) {
                pcap[i] = ff[i].payload_len > pcap[i] ? ff[i].payload_len : (pcap[i] < 0x10000000u ? 8 * pcap[i] + 65536 : 0xFFFFFF00u);
                if (scap[i] < pcap[i]) scap[i] = pcap[i];
                retry = true;
            } else if (ff[i].status == 6 && attempt < 2) { scap[i] = ff[i].n_samples; retry = true; }
            else if (ff[i].status != 0) bad = true;
        }
        if (bad) { s5gpu_set_error("s5gpu_signal_stats_stream: at least one record is corrupt (see stats_out[i].status)"); return S5GPU_ERR_DATA; }
        if (!retry) break;
    }
    return S5GPU_OK;
}

extern "C" int s5gpu_signal_stats_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                                         int sig_method, uint32_t n_q, const double *q, s5gpu_sig_stats_t *stats_out, s5gpu_rec_fields_t *fields_out) {
    const char *who = "s5gpu_signal_stats_stream";
    sigk::Quantiles Q;
    int rc;
    if ((rc = check_quantiles(who, n_q, q, &Q))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len || !stats_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if ((rec_method != S5GPU_REC_NONE && rec_method != S5GPU_REC_ZLIB && rec_method != S5GPU_REC_ZSTD) ||
        (sig_method != S5GPU_SIG_NONE && sig_method != S5GPU_SIG_SVB_ZD && sig_method != S5GPU_SIG_EX_ZD)) {
        s5gpu_set_error("%s: unsupported method", who);
        return S5GPU_ERR_ARG;
    }
    uint64_t b0 = UINT64_MAX, e1 = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec_pos[i] > chunk_bytes || rec_len[i] > chunk_bytes - rec_pos[i]) { s5gpu_set_error("record %u lies outside the chunk", i); return S5GPU_ERR_ARG; }
        b0 = b0 < rec_pos[i] ? b0 : rec_pos[i];
        e1 = e1 > rec_pos[i] + rec_len[i] ? e1 : rec_pos[i] + rec_len[i];
    }
    b0 &= ~15ull;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    std::vector<s5gpu_rec_fields_t> ff;
    // the decoders that keep no payload: zlib / zstd + svb-zd and zlib + ex-zd; every other pair of methods is decoded in full
    const bool np = (sig_method == S5GPU_SIG_SVB_ZD && (rec_method == S5GPU_REC_ZLIB || rec_method == S5GPU_REC_ZSTD)) ||
                    (sig_method == S5GPU_SIG_EX_ZD && rec_method == S5GPU_REC_ZLIB);
    int drc;
    if (np) {
        if ((rc = c->d_in.reserve(e1 - b0 + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_in.p, (const uint8_t *)chunk + b0, e1 - b0, hipMemcpyHostToDevice, c->st));
        drc = s5host::decode_np_framed(c, n, (const uint8_t *)chunk, b0, rec_pos, rec_len, rec_method, sig_method, ff);
    } else {
        std::vector<const void *> rec(n);
        std::vector<size_t> len(n);
        std::vector<s5gpu_rec_desc_t> rd;
        for (uint32_t i = 0; i < n; i++) { rec[i] = (const uint8_t *)chunk + rec_pos[i]; len[i] = rec_len[i]; }
        drc = s5host::decode_resident_framed(c, n, rec.data(), len.data(), rec_method, sig_method, rd, ff, nullptr, (const uint8_t *)chunk + b0, (size_t)(e1 - b0));
    }
    if (drc && drc != S5GPU_ERR_DATA) return drc;
    const std::string data_msg = drc ? s5gpu_last_error() : "";
    // the statistics of what the decode left on the device: a failed record has n_eff = 0, so the kernel reads nothing of it
    if ((rc = c->d_patch.reserve(sizeof(s5gpu_sig_stats_t) * n)) || (rc = c->h_out.reserve(sizeof(s5gpu_sig_stats_t) * (size_t)n + 64))) return rc;
    const sigk::SigRecs R = {(const int16_t *)c->d_sig2.p, (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_off),
                             (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_cap), (const s5gpu_rec_fields_t *)c->d_fields.p,
                             sizeof(s5gpu_rec_desc_t), sizeof(s5gpu_rec_desc_t), n};
    if ((rc = sigk::launch_stats(R, Q, (s5gpu_sig_stats_t *)c->d_patch.p, c->st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_patch.p, sizeof(s5gpu_sig_stats_t) * n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(stats_out, c->h_out.p, sizeof(s5gpu_sig_stats_t) * n);
    if (fields_out) memcpy(fields_out, ff.data(), sizeof(s5gpu_rec_fields_t) * n);
    if (drc) { s5gpu_set_error("%s", data_msg.c_str()); return drc; }
    return S5GPU_OK;
}
