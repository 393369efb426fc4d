// digest_api.hip — host side of the digest calls (include/slow5gpu.h, "sum"): argument checks and the launch of the device entry point, and
// s5gpu_digest_stream / s5gpu_digest_batch: upload -> full decode (the aux bytes are part of a record's canonical form, so the payloads are
// kept) -> k_rec_digest -> a download of 8 bytes per record.  Neither payloads nor signals leave the device.
#include "digest_dev.h"
#include "host_ctx.h"

namespace {

// the digests of what a decode_resident* call left in the context (a failed record: 0), through the pinned staging buffer
int digest_resident(Ctx *c, uint32_t n, uint64_t *digest_out) {
    int rc;
    if ((rc = c->d_patch.reserve(sizeof(uint64_t) * (size_t)n)) || (rc = c->h_out.reserve(sizeof(uint64_t) * (size_t)n + 64))) return rc;
    const digk::DigRecs R = {(const s5gpu_rec_desc_t *)c->d_desc2.p, (const uint8_t *)c->d_pay.p, (const int16_t *)c->d_sig2.p,
                             (const s5gpu_rec_fields_t *)c->d_fields.p, n};
    if ((rc = digk::launch_digest(R, (uint64_t *)c->d_patch.p, c->st))) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_patch.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    memcpy(digest_out, c->h_out.p, sizeof(uint64_t) * n);
    return S5GPU_OK;
}

// the digests of the records the front left resident, at their places in the batch; a record it dropped has digest 0
int digest_front(const char *who, Ctx *c, uint32_t n, const s5host::Resident &R, uint64_t *digest_out, int32_t *status_out) {
    int rc;
    std::vector<uint64_t> dg(R.m == n ? 0 : R.m);
    if ((rc = digest_resident(c, R.m, R.m == n ? digest_out : dg.data()))) return rc;
    if (R.m != n) {
        memset(digest_out, 0, sizeof(uint64_t) * n);
        for (uint32_t k = 0; k < R.m; k++) digest_out[R.cur[k]] = dg[k];
    }
    if (status_out) memcpy(status_out, R.status, sizeof(int32_t) * n);
    if (R.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its digest is 0)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

}  // namespace

extern "C" int s5gpu_digest_dev(uint32_t n, const s5gpu_rec_desc_t *desc, const uint8_t *payload, const int16_t *sig, const s5gpu_rec_fields_t *fields,
                                int sig_method, uint64_t *digest, void *stream) {
    const char *who = "s5gpu_digest_dev";
    if (!s5rules::sig_method_ok(sig_method)) { s5gpu_set_error("%s: unknown signal method %d", who, sig_method); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!desc || !payload || !sig || !fields || !digest) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)payload & 15u) || ((uintptr_t)sig & 15u) || ((uintptr_t)desc & 7u) || ((uintptr_t)fields & 7u) || ((uintptr_t)digest & 7u)) {
        s5gpu_set_error("%s: misaligned argument (payload, sig: 16 bytes; desc, fields, digest: 8)", who);
        return S5GPU_ERR_ARG;
    }
    const digk::DigRecs R = {desc, payload, sig, fields, n};
    return digk::launch_digest(R, digest, (hipStream_t)stream);
}

extern "C" int s5gpu_digest_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                                   int sig_method, uint64_t *digest_out, int32_t *status_out) {
    const char *who = "s5gpu_digest_stream";
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len || !digest_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    uint64_t b0, e1;
    int rc;
    if ((rc = s5rules::chunk_span(who, "record", n, chunk_bytes, rec_pos, rec_len, &b0, &e1))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    s5host::Resident R;
    if ((rc = s5host::resident_chunk(hold.c, who, n, chunk, b0, e1, rec_pos, rec_len, rec_method, sig_method, true, R))) return rc;
    return digest_front(who, hold.c, n, R, digest_out, status_out);
}

extern "C" int s5gpu_digest_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, uint64_t *digest_out,
                                  int32_t *status_out) {
    const char *who = "s5gpu_digest_batch";
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!rec || !rec_len || !digest_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    int rc;
    if ((rc = s5rules::host_records_ok(who, n, rec, rec_len))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    s5host::Resident R;
    if ((rc = s5host::resident_records(hold.c, n, rec, rec_len, rec_method, sig_method, R))) return rc;
    return digest_front(who, hold.c, n, R, digest_out, status_out);
}
