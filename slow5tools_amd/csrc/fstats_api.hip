// fstats_api.hip — host side of the file statistics (include/slow5gpu.h, "stats"): argument checks and launches of the two device entry points,
// and the per-file handle: s5gpu_file_stats_add_stream uploads a file chunk, decodes it (fields + signals only where the methods allow it) and
// adds what the decode left on the device to the handle's accumulator; s5gpu_file_stats_close makes the one download.
#include "fstats_dev.h"
#include "host_ctx.h"

namespace {

struct Handle {
    s5gpu_file_stats_t *d_acc = nullptr;
};

bool methods_ok(int rec_method, int sig_method) {
    return (rec_method == S5GPU_REC_NONE || rec_method == S5GPU_REC_ZLIB || rec_method == S5GPU_REC_ZSTD) &&
           (sig_method == S5GPU_SIG_NONE || sig_method == S5GPU_SIG_SVB_ZD || sig_method == S5GPU_SIG_EX_ZD);
}

// what the last decode of this context left on the device, as the kernels take it
sigk::SigRecs resident(Ctx *c, uint32_t n) {
    return {(const int16_t *)c->d_sig2.p, (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_off),
            (const uint8_t *)c->d_desc2.p + offsetof(s5gpu_rec_desc_t, sig_cap), (const s5gpu_rec_fields_t *)c->d_fields.p,
            sizeof(s5gpu_rec_desc_t), sizeof(s5gpu_rec_desc_t), n};
}

}  // namespace

extern "C" size_t s5gpu_file_stats_bytes(void) { return sizeof(s5gpu_file_stats_t); }

extern "C" int s5gpu_file_stats_reset_dev(s5gpu_file_stats_t *acc, void *stream) {
    if (!acc || ((uintptr_t)acc & 7u)) { s5gpu_set_error("s5gpu_file_stats_reset_dev: NULL or misaligned acc"); return S5GPU_ERR_ARG; }
    return fsk::launch_reset(acc, (hipStream_t)stream);
}

extern "C" int s5gpu_file_stats_accum_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                                          s5gpu_file_stats_t *acc, void *stream) {
    const char *who = "s5gpu_file_stats_accum_dev";
    if (!acc || ((uintptr_t)acc & 7u)) { s5gpu_set_error("%s: NULL or misaligned acc", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!sig || !sig_off || !sig_cap || !fields) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)sig & 15u) || ((uintptr_t)sig_off & 7u) || ((uintptr_t)sig_cap & 3u) || ((uintptr_t)fields & 7u)) {
        s5gpu_set_error("%s: misaligned argument (sig: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    const sigk::SigRecs R = {sig, (const uint8_t *)sig_off, (const uint8_t *)sig_cap, fields, sizeof(uint64_t), sizeof(uint32_t), n};
    return fsk::launch_accum(R, acc, (hipStream_t)stream);
}

extern "C" void *s5gpu_file_stats_open(void) {
    if (s5host::n_devices() == 0) return nullptr;
    s5host::CtxHold hold;
    if (hold.acquire(0)) return nullptr;
    Ctx *c = hold.c;
    Handle *h = new Handle;
    hipError_t e = hipMalloc((void **)&h->d_acc, sizeof(s5gpu_file_stats_t));
    if (e != hipSuccess) {
        s5gpu_set_error("s5gpu_file_stats_open: allocation of the accumulator failed: %s", hipGetErrorString(e));
        delete h;
        return nullptr;
    }
    if (fsk::launch_reset(h->d_acc, c->st) != S5GPU_OK || hipStreamSynchronize(c->st) != hipSuccess) {
        (void)hipFree(h->d_acc);
        delete h;
        return nullptr;
    }
    return h;
}

extern "C" int s5gpu_file_stats_add_stream(void *handle, uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len,
                                           int rec_method, int sig_method, int32_t *status_out) {
    const char *who = "s5gpu_file_stats_add_stream";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    uint64_t b0 = UINT64_MAX, e1 = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec_pos[i] > chunk_bytes || rec_len[i] > chunk_bytes - rec_pos[i]) { s5gpu_set_error("%s: record %u lies outside the chunk", who, i); return S5GPU_ERR_ARG; }
        b0 = b0 < rec_pos[i] ? b0 : rec_pos[i];
        e1 = e1 > rec_pos[i] + rec_len[i] ? e1 : rec_pos[i] + rec_len[i];
    }
    b0 &= ~15ull;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    int rc;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    // the decoders that keep no payload: zlib / zstd + svb-zd and zlib + ex-zd; every other pair of methods is decoded in full
    const bool np = (sig_method == S5GPU_SIG_SVB_ZD && (rec_method == S5GPU_REC_ZLIB || rec_method == S5GPU_REC_ZSTD)) ||
                    (sig_method == S5GPU_SIG_EX_ZD && rec_method == S5GPU_REC_ZLIB);
    if (np) {                                                  // the one upload: a second decode of a part of the batch reads the same bytes
        if ((rc = c->d_in.reserve(e1 - b0 + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_in.p, (const uint8_t *)chunk + b0, e1 - b0, hipMemcpyHostToDevice, c->st));
    }
    std::vector<s5gpu_rec_fields_t> ff;
    std::vector<uint64_t> pos;
    std::vector<uint32_t> len;
    auto decode = [&](uint32_t m, const uint32_t *idx) {
        pos.resize(m); len.resize(m);
        for (uint32_t k = 0; k < m; k++) { pos[k] = rec_pos[idx[k]]; len[k] = rec_len[idx[k]]; }
        if (np) return s5host::decode_np_framed(c, m, (const uint8_t *)chunk, b0, pos.data(), len.data(), rec_method, sig_method, ff);
        std::vector<const void *> rec(m);
        std::vector<size_t> l(m);
        std::vector<s5gpu_rec_desc_t> rd;
        for (uint32_t i = 0; i < m; i++) { rec[i] = (const uint8_t *)chunk + pos[i]; l[i] = len[i]; }
        return s5host::decode_resident_framed(c, m, rec.data(), l.data(), rec_method, sig_method, rd, ff, nullptr, (const uint8_t *)chunk + b0, (size_t)(e1 - b0));
    };
    // Corrupt records must be counted all the same: s5host::decode_dropping_corrupt decodes the batch again without them while records that
    // outgrew their slots are left; the dropped ones are counted here.  What still has status 5 / 6 after the last round is counted as failed by
    // the kernel (n_eff = 0: it counts the record and reads nothing of it).
    std::vector<uint32_t> cur;
    std::vector<int32_t> status(n);
    bool corrupt = false;
    if ((rc = s5host::decode_dropping_corrupt(n, decode, ff, cur, status.data(), &corrupt))) return rc;
    if (status_out) memcpy(status_out, status.data(), sizeof(int32_t) * n);
    const uint32_t m = (uint32_t)cur.size();
    if ((rc = fsk::launch_accum(resident(c, m), h->d_acc, c->st)) || (rc = fsk::launch_add_failed(h->d_acc, n - m, c->st))) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));                      // the next holder of this context overwrites the signals
    if (corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; it is counted in n_failed)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

extern "C" int s5gpu_file_stats_close(void *handle, s5gpu_file_stats_t *out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    auto fetch = [&]() -> int {
        s5host::CtxHold hold;
        int r;
        if ((r = hold.acquire(0))) return r;
        Ctx *c = hold.c;
        if ((r = c->h_out.reserve(sizeof(s5gpu_file_stats_t) + 64))) return r;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, h->d_acc, sizeof(s5gpu_file_stats_t), hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        memcpy(out, c->h_out.p, sizeof(s5gpu_file_stats_t));
        return S5GPU_OK;
    };
    const int rc = h->d_acc && out ? fetch() : S5GPU_OK;
    if (h->d_acc) (void)hipFree(h->d_acc);                      // whatever the download did: the handle ends here
    delete h;
    return rc;
}
