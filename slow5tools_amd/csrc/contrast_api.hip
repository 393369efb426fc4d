// contrast_api.hip — host side of the contrast calls (include/slow5gpu.h, "contrast"; docs/codecs.md §4.23): the histogram's size, argument
// checks and launches of the device entry points, and the per-file handle with two sides: s5gpu_contrast_add_batch is
// s5gpu_pileup_add_batch_whole (pilek::add_batch_whole) into the side's table and histogram, s5gpu_contrast_close runs k_pile_contrast and
// makes the downloads.
#include "pileup_host.h"
#include "fold_dev.h"

namespace {

struct Handle {
    pilek::WholeChain c;
    void *d_acc[2] = {nullptr, nullptr};
    void *d_hist[2] = {nullptr, nullptr};
};

bool bins_ok(const char *who, uint32_t R, int32_t q0, uint32_t shift) {
    if (R == 0 || R > pilek::HIST_RMAX) { s5gpu_set_error("%s: a histogram of %u columns (1 .. 2^22)", who, R); return false; }
    if (q0 < -32768 || q0 > 32767 || shift > pilek::HIST_SHIFT_MAX) { s5gpu_set_error("%s: q0 %d (-32768 .. 32767), shift %u (0 .. 10)", who, q0, shift); return false; }
    return true;
}

void free_handle(Handle *h) {
    for (int s = 0; s < 2; s++) {
        if (h->d_acc[s]) (void)hipFree(h->d_acc[s]);
        if (h->d_hist[s]) (void)hipFree(h->d_hist[s]);
    }
    delete h;
}

}  // namespace

extern "C" size_t s5gpu_pile_hist_bytes(uint32_t R) {
    if (R == 0 || R > pilek::HIST_RMAX) return 0;
    return sizeof(s5gpu_pile_hist_head_t) + 4u * pilek::HIST_BINS * (size_t)R;
}

extern "C" int s5gpu_pile_hist_reset_dev(void *hist, uint32_t R, int32_t q0, uint32_t shift, void *stream) {
    const char *who = "s5gpu_pile_hist_reset_dev";
    if (!bins_ok(who, R, q0, shift)) return S5GPU_ERR_ARG;
    if (!hist || ((uintptr_t)hist & 15u)) { s5gpu_set_error("%s: NULL or misaligned hist (16 bytes)", who); return S5GPU_ERR_ARG; }
    return pilek::launch_hist_reset(hist, R, q0, shift, (hipStream_t)stream);
}

extern "C" int s5gpu_pile_hist_accum_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, uint32_t R,
                                              const int32_t *lo, const int32_t *hi, const int32_t *status, void *work, size_t work_bytes, void *hist, void *stream) {
    pilek::PileLongArgs A;
    A.n = n; A.queries = queries; A.first = first; A.qlen = qlen; A.total_rows = total_rows; A.ref = nullptr; A.R = R; A.lo = lo; A.hi = hi; A.status = status;
    A.events = nullptr; A.ev_skip = 0u; A.work = work; A.acc = nullptr;
    return pilek::accum_long_checked("s5gpu_pile_hist_accum_long_dev", A, work_bytes, hist, true, (hipStream_t)stream);
}

extern "C" int s5gpu_pile_contrast_dev(const void *hist_a, const void *hist_b, const void *acc_a, const void *acc_b, uint32_t R, s5gpu_pile_contrast_t *out,
                                       void *stream) {
    const char *who = "s5gpu_pile_contrast_dev";
    if (R == 0 || R > pilek::HIST_RMAX) { s5gpu_set_error("%s: histograms of %u columns (1 .. 2^22)", who, R); return S5GPU_ERR_ARG; }
    if (!hist_a || !hist_b || !out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if ((acc_a == nullptr) != (acc_b == nullptr)) { s5gpu_set_error("%s: one table without the other", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)hist_a & 15u) || ((uintptr_t)hist_b & 15u) || ((uintptr_t)acc_a & 15u) || ((uintptr_t)acc_b & 15u) || ((uintptr_t)out & 7u)) {
        s5gpu_set_error("%s: misaligned argument (hist, acc: 16 bytes; out: 8)", who);
        return S5GPU_ERR_ARG;
    }
    return pilek::launch_contrast(hist_a, hist_b, acc_a, acc_b, R, out, (hipStream_t)stream);
}

extern "C" void *s5gpu_contrast_open(const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, size_t scratch_max,
                                     const int16_t *ref_host, uint32_t R, int32_t q0, uint32_t shift) {
    const char *who = "s5gpu_contrast_open";
    if (pilek::whole_open_check(who, ep, mp, bp, ref_host, R)) return nullptr;
    if (!bins_ok(who, R, q0, shift)) return nullptr;
    if (s5host::n_devices() == 0) { s5gpu_set_error("%s: no device", who); return nullptr; }
    Handle *h = new Handle;
    h->c.ep = *ep; h->c.mp = *mp; h->c.mp.want_start = 1; h->c.bp = *bp; h->c.scratch_max = scratch_max;
    h->c.ref.assign(ref_host, ref_host + R);
    for (int s = 0; s < 2; s++) {
        h->d_acc[s] = s5host::acc_open(who, s5gpu_pileup_bytes(R), [R](void *acc, hipStream_t st) { return pilek::launch_reset(acc, R, st); });
        h->d_hist[s] = s5host::acc_open(who, s5gpu_pile_hist_bytes(R), [=](void *hist, hipStream_t st) { return pilek::launch_hist_reset(hist, R, q0, shift, st); });
        if (!h->d_acc[s] || !h->d_hist[s]) { free_handle(h); return nullptr; }
    }
    return h;
}

extern "C" int s5gpu_contrast_add_batch(void *handle, int side, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                        s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out) {
    const char *who = "s5gpu_contrast_add_batch";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (side != 0 && side != 1) { s5gpu_set_error("%s: side %d (0 or 1)", who, side); return S5GPU_ERR_ARG; }
    h->c.started = true;
    return pilek::add_batch_whole(who, h->c, h->d_acc[side], h->d_hist[side], nullptr, n, rec, rec_len, rec_method, sig_method, map_rows_out, ext_rows_out, status_out);
}

extern "C" int s5gpu_contrast_set_refine(void *handle, const s5gpu_refine_params_t *rp) {
    const char *who = "s5gpu_contrast_set_refine";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    return pilek::whole_set_refine(who, h->c, rp);
}

extern "C" int s5gpu_contrast_close(void *handle, void *acc_a_out, void *acc_b_out, s5gpu_pile_contrast_t *rows_out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    const uint32_t R = (uint32_t)h->c.ref.size();
    const size_t row_bytes = sizeof(s5gpu_pile_contrast_t) * (size_t)R;
    void *d_rows = nullptr;
    auto fetch = [&]() -> int {
        s5host::CtxHold hold;
        int r;
        if ((r = hold.acquire(0))) return r;
        Ctx *c = hold.c;
        HIP_TRY(hipMalloc(&d_rows, row_bytes));
        if ((r = pilek::launch_contrast(h->d_hist[0], h->d_hist[1], h->d_acc[0], h->d_acc[1], R, (s5gpu_pile_contrast_t *)d_rows, c->st))) return r;
        // (straight into the caller's buffers, as s5gpu_pileup_close: a table may be gigabytes)
        HIP_TRY(hipMemcpyAsync(rows_out, d_rows, row_bytes, hipMemcpyDeviceToHost, c->st));
        if (acc_a_out) HIP_TRY(hipMemcpyAsync(acc_a_out, h->d_acc[0], s5gpu_pileup_bytes(R), hipMemcpyDeviceToHost, c->st));
        if (acc_b_out) HIP_TRY(hipMemcpyAsync(acc_b_out, h->d_acc[1], s5gpu_pileup_bytes(R), hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        return S5GPU_OK;
    };
    const int rc = rows_out ? fetch() : S5GPU_OK;
    if (d_rows) (void)hipFree(d_rows);
    free_handle(h);                                                        // whatever the downloads did: the handle ends here
    return rc;
}

// §4.26: both sides' table and histogram folded onto K classes on the device, the unchanged k_pile_contrast over the K rows
extern "C" int s5gpu_contrast_close_folded(void *handle, const uint32_t *cls_host, uint32_t K, void *acc_a_out, void *acc_b_out, s5gpu_pile_contrast_t *rows_out) {
    const char *who = "s5gpu_contrast_close_folded";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    const uint32_t R = (uint32_t)h->c.ref.size();
    void *d_cls = nullptr, *d_rows = nullptr, *d_acc[2] = {nullptr, nullptr}, *d_hist[2] = {nullptr, nullptr};
    auto fetch = [&]() -> int {
        if (!cls_host || !rows_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
        if (K == 0 || K > pilek::HIST_RMAX) { s5gpu_set_error("%s: %u classes (1 .. 2^22)", who, K); return S5GPU_ERR_ARG; }
        s5host::CtxHold hold;
        int r;
        if ((r = hold.acquire(0))) return r;
        Ctx *c = hold.c;
        s5gpu_pile_hist_head_t head;                                       // q0 and shift: the sides' own
        HIP_TRY(hipMemcpy(&head, h->d_hist[0], sizeof head, hipMemcpyDeviceToHost));
        const size_t row_bytes = sizeof(s5gpu_pile_contrast_t) * (size_t)K;
        HIP_TRY(hipMalloc(&d_cls, sizeof(uint32_t) * (size_t)R));
        HIP_TRY(hipMalloc(&d_rows, row_bytes));
        HIP_TRY(hipMemcpyAsync(d_cls, cls_host, sizeof(uint32_t) * (size_t)R, hipMemcpyHostToDevice, c->st));
        for (int s = 0; s < 2; s++) {
            HIP_TRY(hipMalloc(&d_acc[s], s5gpu_pileup_bytes(K)));
            HIP_TRY(hipMalloc(&d_hist[s], s5gpu_pile_hist_bytes(K)));
            if ((r = pilek::launch_reset(d_acc[s], K, c->st))) return r;
            if ((r = pilek::launch_hist_reset(d_hist[s], K, head.q0, head.shift, c->st))) return r;
            if ((r = pilek::fold_checked(who, h->d_acc[s], R, (const uint32_t *)d_cls, K, d_acc[s], c->st))) return r;
            if ((r = pilek::hist_fold_checked(who, h->d_hist[s], R, (const uint32_t *)d_cls, K, d_hist[s], c->st))) return r;
        }
        if ((r = pilek::launch_contrast(d_hist[0], d_hist[1], d_acc[0], d_acc[1], K, (s5gpu_pile_contrast_t *)d_rows, c->st))) return r;
        HIP_TRY(hipMemcpyAsync(rows_out, d_rows, row_bytes, hipMemcpyDeviceToHost, c->st));
        if (acc_a_out) HIP_TRY(hipMemcpyAsync(acc_a_out, d_acc[0], s5gpu_pileup_bytes(K), hipMemcpyDeviceToHost, c->st));
        if (acc_b_out) HIP_TRY(hipMemcpyAsync(acc_b_out, d_acc[1], s5gpu_pileup_bytes(K), hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        return S5GPU_OK;
    };
    const int rc = fetch();
    for (void *p : {d_cls, d_rows, d_acc[0], d_acc[1], d_hist[0], d_hist[1]})
        if (p) (void)hipFree(p);
    free_handle(h);                                                        // whatever the fold did: the handle ends here
    return rc;
}
