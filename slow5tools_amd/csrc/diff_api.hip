// diff_api.hip — host side of the diff calls (include/slow5gpu.h, "diff"): argument checks and the launch of the device entry point, and the
// per-file handle.  A Ctx holds one decode, so s5gpu_diff_add_batch decodes A in full, copies what the decode left (signal slab, payload slab,
// descriptors, fields) device to device into the handle's own buffers, decodes B in the same context and runs k_sig_diff over the two:
// one extra pass over A's decoded bytes.  Nothing but n x 80 bytes of rows comes back per batch, and the accumulator once at the close.
#include "diff_dev.h"
#include "host_ctx.h"

namespace {

struct Handle {
    s5gpu_diff_acc_t *d_acc = nullptr;
    Buf sig, pay, desc, fields;        // side A of the batch at hand
    Buf pairs, rows;
};

// a decoded batch whose descriptors are the decoder's own table
dfk::Side side_of(const void *sig, const void *desc, const void *fields, const void *pay, uint32_t n) {
    const uint8_t *d = (const uint8_t *)desc;
    const uint32_t s = sizeof(s5gpu_rec_desc_t);
    const sigk::SigRecs S = s5host::sig_recs_of(sig, desc, fields, n);
    return {S.sig, S.off, S.cap, S.fields, (const uint8_t *)pay, d + offsetof(s5gpu_rec_desc_t, pay_off), d + offsetof(s5gpu_rec_desc_t, pay_cap), s, s, s, s, n};
}

int check_side(const char *who, const char *name, const s5gpu_diff_side_t *S) {
    if (S->n == 0) return S5GPU_OK;                                      // every pair that names it is a BAD_PAIR: nothing of it is read
    if (!S->sig || !S->sig_off || !S->sig_cap || !S->fields || (S->payload && (!S->pay_off || !S->pay_cap))) {
        s5gpu_set_error("%s: NULL member of side %s", who, name);
        return S5GPU_ERR_ARG;
    }
    if (((uintptr_t)S->sig & 15u) || ((uintptr_t)S->sig_off & 7u) || ((uintptr_t)S->sig_cap & 3u) || ((uintptr_t)S->fields & 7u) ||
        ((uintptr_t)S->payload & 15u) || (S->payload && (((uintptr_t)S->pay_off & 7u) || ((uintptr_t)S->pay_cap & 3u)))) {
        s5gpu_set_error("%s: misaligned member of side %s (sig, payload: 16 bytes)", who, name);
        return S5GPU_ERR_ARG;
    }
    return S5GPU_OK;
}

dfk::Side plain_side(const s5gpu_diff_side_t *S) {
    return {S->sig, (const uint8_t *)S->sig_off, (const uint8_t *)S->sig_cap, S->fields, S->payload, (const uint8_t *)S->pay_off, (const uint8_t *)S->pay_cap,
            sizeof(uint64_t), sizeof(uint32_t), sizeof(uint64_t), sizeof(uint32_t), S->n};
}

s5gpu_sig_diff_t failed_row(int32_t sa, int32_t sb) {
    s5gpu_sig_diff_t r;
    memset(&r, 0, sizeof r);
    r.status_a = sa; r.status_b = sb;
    r.flags = S5GPU_DIFF_FAILED;
    r.first_diff = S5GPU_DIFF_NONE; r.max_at = S5GPU_DIFF_NONE;
    return r;
}

}  // namespace

extern "C" size_t s5gpu_diff_acc_bytes(void) { return sizeof(s5gpu_diff_acc_t); }

extern "C" int s5gpu_diff_acc_reset_dev(s5gpu_diff_acc_t *acc, void *stream) {
    if (!acc || ((uintptr_t)acc & 7u)) { s5gpu_set_error("s5gpu_diff_acc_reset_dev: NULL or misaligned acc"); return S5GPU_ERR_ARG; }
    return dfk::launch_reset(acc, (hipStream_t)stream);
}

extern "C" int s5gpu_signal_diff_dev(uint32_t n_pairs, const uint32_t *pair_a, const uint32_t *pair_b, const s5gpu_diff_side_t *A, const s5gpu_diff_side_t *B,
                                     s5gpu_sig_diff_t *out, s5gpu_diff_acc_t *acc, void *stream) {
    const char *who = "s5gpu_signal_diff_dev";
    if (((uintptr_t)out & 7u) || ((uintptr_t)acc & 7u)) { s5gpu_set_error("%s: misaligned out or acc (8 bytes)", who); return S5GPU_ERR_ARG; }
    if (n_pairs == 0) return S5GPU_OK;
    if (!pair_a || !pair_b || !A || !B) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)pair_a & 3u) || ((uintptr_t)pair_b & 3u)) { s5gpu_set_error("%s: misaligned pair list", who); return S5GPU_ERR_ARG; }
    int rc;
    if ((rc = check_side(who, "A", A)) || (rc = check_side(who, "B", B))) return rc;
    return dfk::launch_diff(n_pairs, pair_a, pair_b, plain_side(A), plain_side(B), out, acc, (hipStream_t)stream);
}

extern "C" void *s5gpu_diff_open(void) {
    Handle *h = new Handle;
    h->d_acc = (s5gpu_diff_acc_t *)s5host::acc_open("s5gpu_diff_open", sizeof(s5gpu_diff_acc_t),
                                                     [](void *acc, hipStream_t st) { return dfk::launch_reset((s5gpu_diff_acc_t *)acc, st); });
    if (!h->d_acc) { delete h; return nullptr; }
    return h;
}

extern "C" int s5gpu_diff_add_batch(void *handle, uint32_t n, const void *const *rec_a, const size_t *len_a, int rec_a_method, int sig_a_method,
                                    const void *const *rec_b, const size_t *len_b, int rec_b_method, int sig_b_method, s5gpu_sig_diff_t *out,
                                    int32_t *status_a, int32_t *status_b) {
    const char *who = "s5gpu_diff_add_batch";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!s5rules::methods_ok(rec_a_method, sig_a_method) || !s5rules::methods_ok(rec_b_method, sig_b_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!rec_a || !len_a || !rec_b || !len_b) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    int rc;
    if ((rc = s5rules::host_records_ok(who, n, rec_a, len_a)) || (rc = s5rules::host_records_ok(who, n, rec_b, len_b))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5host::CtxHold hold;
    if ((rc = hold.acquire(0))) return rc;
    Ctx *c = hold.c;

    // A: decoded in full, then moved out of the context's way
    s5host::Resident RA, RB;                                               // (one at a time: RA's arrays are copied before B is decoded)
    if ((rc = s5host::resident_records(c, n, rec_a, len_a, rec_a_method, sig_a_method, RA))) return rc;
    const uint32_t m_a = RA.m;
    const std::vector<uint32_t> cur_a(RA.cur, RA.cur + m_a);               // (B's decode takes the context's host arrays over)
    const std::vector<int32_t> st_a(RA.status, RA.status + n);
    if (m_a) {
        const s5gpu_rec_desc_t &last = RA.rd[m_a - 1];                        // the slots lie in record order (decode_resident)
        const uint64_t so = last.sig_off + up((uint64_t)last.sig_cap + 8, 8), po = last.pay_off + up((uint64_t)last.pay_cap + 16, 16);
        if ((rc = h->sig.reserve(so * 2 + 64)) || (rc = h->pay.reserve(po + 64)) || (rc = h->desc.reserve(sizeof(s5gpu_rec_desc_t) * m_a)) ||
            (rc = h->fields.reserve(sizeof(s5gpu_rec_fields_t) * m_a)))
            return rc;
        HIP_TRY(hipMemcpyAsync(h->sig.p, c->d_sig2.p, so * 2, hipMemcpyDeviceToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(h->pay.p, c->d_pay.p, po, hipMemcpyDeviceToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(h->desc.p, c->d_desc2.p, sizeof(s5gpu_rec_desc_t) * m_a, hipMemcpyDeviceToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(h->fields.p, c->d_fields.p, sizeof(s5gpu_rec_fields_t) * m_a, hipMemcpyDeviceToDevice, c->st));
    }
    // B: stays where the decoder left it
    if ((rc = s5host::resident_records(c, n, rec_b, len_b, rec_b_method, sig_b_method, RB))) return rc;
    const uint32_t m_b = RB.m;
    if (status_a) memcpy(status_a, st_a.data(), sizeof(int32_t) * n);
    if (status_b) memcpy(status_b, RB.status, sizeof(int32_t) * n);

    // the pairs whose two records are resident; a pair with a record the front dropped is FAILED here, with the decoder's statuses
    std::vector<uint32_t> at_a(n, 0xFFFFFFFFu), at_b(n, 0xFFFFFFFFu), sent;
    for (uint32_t k = 0; k < m_a; k++) at_a[cur_a[k]] = k;
    for (uint32_t k = 0; k < m_b; k++) at_b[RB.cur[k]] = k;
    for (uint32_t i = 0; i < n; i++)
        if (at_a[i] != 0xFFFFFFFFu && at_b[i] != 0xFFFFFFFFu) sent.push_back(i);
    const uint32_t ns = (uint32_t)sent.size();
    if (ns) {
        if ((rc = c->h_in.reserve(8ull * ns + 64)) || (rc = c->h_out.reserve(sizeof(s5gpu_sig_diff_t) * (size_t)ns + 64)) || (rc = h->pairs.reserve(8ull * ns)) ||
            (rc = h->rows.reserve(sizeof(s5gpu_sig_diff_t) * (size_t)ns)))
            return rc;
        uint32_t *hp = (uint32_t *)c->h_in.p;
        for (uint32_t k = 0; k < ns; k++) { hp[k] = at_a[sent[k]]; hp[ns + k] = at_b[sent[k]]; }
        HIP_TRY(hipMemcpyAsync(h->pairs.p, hp, 8ull * ns, hipMemcpyHostToDevice, c->st));
        const dfk::Side A = side_of(h->sig.p, h->desc.p, h->fields.p, h->pay.p, m_a);
        const dfk::Side B = side_of(c->d_sig2.p, c->d_desc2.p, c->d_fields.p, c->d_pay.p, m_b);
        if ((rc = dfk::launch_diff(ns, (const uint32_t *)h->pairs.p, (const uint32_t *)h->pairs.p + ns, A, B, (s5gpu_sig_diff_t *)h->rows.p, h->d_acc, c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, h->rows.p, sizeof(s5gpu_sig_diff_t) * (size_t)ns, hipMemcpyDeviceToHost, c->st));
    }
    if ((rc = dfk::launch_add_failed(h->d_acc, n - ns, c->st))) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));                                  // the next holder of this context overwrites B
    if (out) {
        for (uint32_t i = 0; i < n; i++) out[i] = failed_row(st_a[i], RB.status[i]);
        const s5gpu_sig_diff_t *rows = (const s5gpu_sig_diff_t *)c->h_out.p;
        for (uint32_t k = 0; k < ns; k++) out[sent[k]] = rows[k];
    }
    if (RA.corrupt || RB.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; its pair is FAILED and counted in n_failed)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

extern "C" int s5gpu_diff_close(void *handle, s5gpu_diff_acc_t *acc_out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    const int rc = s5host::acc_close(h->d_acc, sizeof(s5gpu_diff_acc_t), acc_out);
    h->sig.release(); h->pay.release(); h->desc.release(); h->fields.release(); h->pairs.release(); h->rows.release();
    delete h;
    return rc;
}
