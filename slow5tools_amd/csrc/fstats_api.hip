// fstats_api.hip — host side of the file statistics (include/slow5gpu.h, "stats"): argument checks and launches of the two device entry points,
// and the per-file handle: s5gpu_file_stats_add_stream uploads a file chunk, decodes it (fields + signals only where the methods allow it) and
// adds what the decode left on the device to the handle's accumulator; s5gpu_file_stats_close makes the one download.
#include "fstats_dev.h"
#include "host_ctx.h"

namespace {

struct Handle {
    s5gpu_file_stats_t *d_acc = nullptr;
};

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
    Handle *h = new Handle;
    h->d_acc = (s5gpu_file_stats_t *)s5host::acc_open("s5gpu_file_stats_open", sizeof(s5gpu_file_stats_t),
                                                       [](void *acc, hipStream_t st) { return fsk::launch_reset((s5gpu_file_stats_t *)acc, st); });
    if (!h->d_acc) { delete h; return nullptr; }
    return h;
}

extern "C" int s5gpu_file_stats_add_stream(void *handle, uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len,
                                           int rec_method, int sig_method, int32_t *status_out) {
    const char *who = "s5gpu_file_stats_add_stream";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    uint64_t b0, e1;
    int rc;
    if ((rc = s5rules::chunk_span(who, "record", n, chunk_bytes, rec_pos, rec_len, &b0, &e1))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    // Corrupt records must be counted all the same: the front decodes the batch again without them while records that outgrew their slots are
    // left; the dropped ones are counted here.  What still has status 5 / 6 after the last round is counted as failed by the kernel
    // (n_eff = 0: it counts the record and reads nothing of it).
    s5host::Resident R;
    if ((rc = s5host::resident_chunk(c, who, n, chunk, b0, e1, rec_pos, rec_len, rec_method, sig_method, false, R))) return rc;
    if (status_out) memcpy(status_out, R.status, sizeof(int32_t) * n);
    if ((rc = fsk::launch_accum(s5host::resident_sig_recs(c, R.m), h->d_acc, c->st)) || (rc = fsk::launch_add_failed(h->d_acc, n - R.m, c->st))) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));                      // the next holder of this context overwrites the signals
    if (R.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; it is counted in n_failed)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

extern "C" int s5gpu_file_stats_close(void *handle, s5gpu_file_stats_t *out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    const int rc = s5host::acc_close(h->d_acc, sizeof(s5gpu_file_stats_t), out);
    delete h;
    return rc;
}
