// digest_api.hip — host side of the digest calls (include/slow5gpu.h, "sum"): argument checks and the launch of the device entry point, and
// s5gpu_digest_stream / s5gpu_digest_batch: upload -> full decode (the aux bytes are part of a record's canonical form, so the payloads are
// kept) -> k_rec_digest -> a download of 8 bytes per record.  Neither payloads nor signals leave the device.
#include "digest_dev.h"
#include "host_ctx.h"

namespace {

bool methods_ok(int rec_method, int sig_method) {
    return (rec_method == S5GPU_REC_NONE || rec_method == S5GPU_REC_ZLIB || rec_method == S5GPU_REC_ZSTD) &&
           (sig_method == S5GPU_SIG_NONE || sig_method == S5GPU_SIG_SVB_ZD || sig_method == S5GPU_SIG_EX_ZD);
}

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

// decode (framed: the records lie in [base, base + bytes), uploaded as it is) + digest of n host records
int digest_host_records(const char *who, uint32_t n, const void *const *rec, const size_t *len, int rec_method, int sig_method, const uint8_t *base,
                        size_t bytes, uint64_t *digest_out, int32_t *status_out) {
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    int rc;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;
    std::vector<s5gpu_rec_desc_t> rd;
    std::vector<s5gpu_rec_fields_t> ff;
    auto decode = [&](uint32_t m, const void *const *r, const size_t *l) {
        return base ? s5host::decode_resident_framed(c, m, r, l, rec_method, sig_method, rd, ff, nullptr, base, bytes)
                    : s5host::decode_resident(c, m, r, l, rec_method, sig_method, rd, ff, nullptr);
    };
    const int drc = decode(n, rec, len);
    if (drc && drc != S5GPU_ERR_DATA) return drc;
    if (status_out) for (uint32_t i = 0; i < n; i++) status_out[i] = ff[i].status;
    bool unfinished = false;
    for (uint32_t i = 0; i < n; i++) unfinished |= ff[i].status == 5 || ff[i].status == 6;
    if (!unfinished) {
        if ((rc = digest_resident(c, n, digest_out))) return rc;
    } else {
        // The decode stops at the first attempt that meets a corrupt record, before it has redone the records that outgrew their guessed slots
        // (status 5 / 6).  The other records' results must be valid all the same: the batch is decoded again without the corrupt ones.
        std::vector<uint32_t> keep;
        std::vector<const void *> r2;
        std::vector<size_t> l2;
        for (uint32_t i = 0; i < n; i++) {
            digest_out[i] = 0;
            if (ff[i].status == 0 || ff[i].status == 5 || ff[i].status == 6) { keep.push_back(i); r2.push_back(rec[i]); l2.push_back(len[i]); }
        }
        const uint32_t m = (uint32_t)keep.size();
        const int drc2 = decode(m, r2.data(), l2.data());
        if (drc2 && drc2 != S5GPU_ERR_DATA) return drc2;
        std::vector<uint64_t> dg(m);
        if ((rc = digest_resident(c, m, dg.data()))) return rc;
        for (uint32_t k = 0; k < m; k++) {
            digest_out[keep[k]] = dg[k];
            if (status_out) status_out[keep[k]] = ff[k].status;
        }
    }
    if (drc) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its digest is 0)", who); return drc; }
    return S5GPU_OK;
}

}  // namespace

extern "C" int s5gpu_digest_dev(uint32_t n, const s5gpu_rec_desc_t *desc, const uint8_t *payload, const int16_t *sig, const s5gpu_rec_fields_t *fields,
                                int sig_method, uint64_t *digest, void *stream) {
    const char *who = "s5gpu_digest_dev";
    if (sig_method != S5GPU_SIG_NONE && sig_method != S5GPU_SIG_SVB_ZD && sig_method != S5GPU_SIG_EX_ZD) {
        s5gpu_set_error("%s: unknown signal method %d", who, sig_method);
        return S5GPU_ERR_ARG;
    }
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
    if (!methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!chunk || !rec_pos || !rec_len || !digest_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    uint64_t b0 = UINT64_MAX, e1 = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (rec_pos[i] > chunk_bytes || rec_len[i] > chunk_bytes - rec_pos[i]) { s5gpu_set_error("%s: record %u lies outside the chunk", who, i); return S5GPU_ERR_ARG; }
        b0 = b0 < rec_pos[i] ? b0 : rec_pos[i];
        e1 = e1 > rec_pos[i] + rec_len[i] ? e1 : rec_pos[i] + rec_len[i];
    }
    b0 &= ~15ull;
    std::vector<const void *> rec(n);
    std::vector<size_t> len(n);
    for (uint32_t i = 0; i < n; i++) { rec[i] = (const uint8_t *)chunk + rec_pos[i]; len[i] = rec_len[i]; }
    return digest_host_records(who, n, rec.data(), len.data(), rec_method, sig_method, (const uint8_t *)chunk + b0, (size_t)(e1 - b0), digest_out, status_out);
}

extern "C" int s5gpu_digest_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, uint64_t *digest_out,
                                  int32_t *status_out) {
    const char *who = "s5gpu_digest_batch";
    if (!methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!rec || !rec_len || !digest_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    for (uint32_t i = 0; i < n; i++)
        if (!rec[i] && rec_len[i]) { s5gpu_set_error("%s: record %u is NULL", who, i); return S5GPU_ERR_ARG; }
    return digest_host_records(who, n, rec, rec_len, rec_method, sig_method, nullptr, 0, digest_out, status_out);
}
