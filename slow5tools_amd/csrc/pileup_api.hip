// pileup_api.hip — host side of the pileup calls (include/slow5gpu.h, "pileup"; docs/codecs.md §4.18): the accumulator's size, argument
// checks and launches of the two device entry points, and the per-file handle: s5gpu_pileup_add_batch runs the chain of s5gpu_align_batch
// (the front of dtw_host.h -> sDTW with the start -> the paths -> the query's event rows gathered) and adds the batch to the handle's
// accumulator with k_pileup; the rows and statuses are all that comes back.  s5gpu_pileup_close makes the one download of the table.
// Whole reads (§4.22): the ragged call, and a handle of a second kind whose add runs the device side of s5gpu_extend_batch (band_host.h)
// and adds the ragged paths it leaves on the device.  The checks of a ragged call and that add are shared with contrast_api.hip and
// sites_api.hip (pileup_host.h), which feed a level histogram (§4.23) and the site matrix (§4.25) from the same run.
#include "pileup_host.h"
#include "fold_dev.h"

namespace {

struct Handle {
    bool whole = false;                                                    // opened by s5gpu_pileup_open_whole: c.bp and c.scratch_max count, wmax does not
    pilek::WholeChain c;
    void *d_acc = nullptr;
    uint32_t wmax = 0;
};

bool acc_ok(const char *who, const void *acc, uint32_t R) {
    if (R == 0 || R > pilek::RMAX) { s5gpu_set_error("%s: a table of %u columns (1 .. 2^26)", who, R); return false; }
    if (!acc || ((uintptr_t)acc & 15u)) { s5gpu_set_error("%s: NULL or misaligned acc (16 bytes)", who); return false; }
    return true;
}

}  // namespace

extern "C" size_t s5gpu_pileup_bytes(uint32_t R) {
    if (R == 0 || R > pilek::RMAX) return 0;
    return sizeof(s5gpu_pile_total_t) + sizeof(s5gpu_pile_col_t) * (size_t)R;
}

extern "C" int s5gpu_pileup_reset_dev(void *acc, uint32_t R, void *stream) {
    if (!acc_ok("s5gpu_pileup_reset_dev", acc, R)) return S5GPU_ERR_ARG;
    return pilek::launch_reset(acc, R, (hipStream_t)stream);
}

extern "C" int s5gpu_pileup_accum_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                                      const int32_t *lo, const int32_t *hi, const int32_t *status, const s5gpu_event_t *events, void *acc, void *stream) {
    const char *who = "s5gpu_pileup_accum_dev";
    if (qpitch == 0 || qpitch > pilek::QMAX) { s5gpu_set_error("%s: a pitch of %u values (1 .. %u)", who, qpitch, pilek::QMAX); return S5GPU_ERR_ARG; }
    if (!acc_ok(who, acc, R)) return S5GPU_ERR_ARG;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !lo || !hi || !status) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)queries & 1u) || ((uintptr_t)qlen & 3u) || ((uintptr_t)ref & 1u) || ((uintptr_t)lo & 3u) || ((uintptr_t)hi & 3u) ||
        ((uintptr_t)status & 3u) || ((uintptr_t)events & 15u)) {
        s5gpu_set_error("%s: misaligned argument (events: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    pilek::PileArgs A;
    A.queries = queries; A.qpitch = qpitch; A.qlen = qlen; A.ref = ref; A.R = R; A.lo = lo; A.hi = hi; A.status = status; A.events = events; A.acc = acc;
    return pilek::launch_pileup(n, A, (hipStream_t)stream);
}

extern "C" void *s5gpu_pileup_open(const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, uint32_t wmax, const int16_t *ref_host, uint32_t R) {
    const char *who = "s5gpu_pileup_open";
    if (dtwk::map_front_check(who, 0, nullptr, nullptr, S5GPU_REC_NONE, S5GPU_SIG_NONE, ep, mp, ref_host, R, true)) return nullptr;
    if (dtwk::check_wmax(who, wmax)) return nullptr;
    if (R > pilek::RMAX) { s5gpu_set_error("%s: a table of %u columns (1 .. 2^26)", who, R); return nullptr; }
    if (dtwk::path_scratch_check(who, mp->qmax, wmax)) return nullptr;
    if (s5host::n_devices() == 0) { s5gpu_set_error("%s: no device", who); return nullptr; }
    Handle *h = new Handle;
    h->c.ep = *ep; h->c.mp = *mp; h->c.mp.want_start = 1; h->wmax = wmax;
    h->c.ref.assign(ref_host, ref_host + R);
    h->d_acc = s5host::acc_open(who, s5gpu_pileup_bytes(R), [R](void *acc, hipStream_t st) { return pilek::launch_reset(acc, R, st); });
    if (!h->d_acc) { delete h; return nullptr; }
    return h;
}

extern "C" int s5gpu_pileup_add_batch(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                      s5gpu_map_row_t *rows_out, int32_t *status_out) {
    const char *who = "s5gpu_pileup_add_batch";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (h->whole) { s5gpu_set_error("%s: the handle is one of s5gpu_pileup_open_whole", who); return S5GPU_ERR_ARG; }
    const uint32_t R = (uint32_t)h->c.ref.size(), qmax = h->c.mp.qmax;
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, &h->c.ep, &h->c.mp, h->c.ref.data(), R, true))) return rc;
    if (n == 0) return S5GPU_OK;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, &h->c.ep, &h->c.mp, h->c.ref.data(), R, F))) return rc;
    Ctx *c = F.hold.c;
    // in c->d_gather: the rows and the path statuses, which come back, and lo, hi and the events, which do not
    const dtwk::PathTail T = dtwk::path_layout(F.m, qmax, true);
    if (F.m) {
        if ((rc = dtwk::path_tail(F, &h->c.mp, h->wmax, R, true, T, T.o_lo))) return rc;
        const uint8_t *dg = (const uint8_t *)c->d_gather.p;
        if ((rc = s5gpu_pileup_accum_dev(F.m, F.d_q, qmax, F.d_ql, F.d_ref, R, (const int32_t *)(dg + T.o_lo), (const int32_t *)(dg + T.o_hi),
                                         (const int32_t *)(dg + T.o_pst), (const s5gpu_event_t *)(dg + T.o_ev), h->d_acc, c->st)))
            return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, T.o_lo, hipMemcpyDeviceToHost, c->st));
    }
    if ((rc = pilek::launch_add_skipped(h->d_acc, n - F.m, c->st))) return rc;   // the records that were dropped
    HIP_TRY(hipStreamSynchronize(c->st));                                  // the next holder of this context overwrites the batch
    const uint8_t *hb = (const uint8_t *)c->h_out.p;
    dtwk::scatter_rows(F, n, (const s5gpu_map_row_t *)hb, (const int32_t *)(hb + T.o_pst), rows_out);
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; it counts in reads_skipped)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

extern "C" int s5gpu_pileup_close(void *handle, void *acc_out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    // (straight into the caller's buffer: a table may be gigabytes, too much for the pinned staging buffer)
    const int rc = s5host::acc_close(h->d_acc, s5gpu_pileup_bytes((uint32_t)h->c.ref.size()), acc_out, true);
    delete h;
    return rc;
}

// §4.26: the table folded onto K classes on the device, and only the K columns downloaded
extern "C" int s5gpu_pileup_close_folded(void *handle, const uint32_t *cls_host, uint32_t K, void *acc_out) {
    const char *who = "s5gpu_pileup_close_folded";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    const uint32_t R = (uint32_t)h->c.ref.size();
    void *d_cls = nullptr, *d_out = nullptr;
    auto fetch = [&]() -> int {
        if (!cls_host || !acc_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
        if (K == 0 || K > pilek::RMAX) { s5gpu_set_error("%s: %u classes (1 .. 2^26)", who, K); return S5GPU_ERR_ARG; }
        s5host::CtxHold hold;
        int r;
        if ((r = hold.acquire(0))) return r;
        Ctx *c = hold.c;
        HIP_TRY(hipMalloc(&d_cls, sizeof(uint32_t) * (size_t)R));
        HIP_TRY(hipMalloc(&d_out, s5gpu_pileup_bytes(K)));
        HIP_TRY(hipMemcpyAsync(d_cls, cls_host, sizeof(uint32_t) * (size_t)R, hipMemcpyHostToDevice, c->st));
        if ((r = pilek::launch_reset(d_out, K, c->st))) return r;
        if ((r = pilek::fold_checked(who, h->d_acc, R, (const uint32_t *)d_cls, K, d_out, c->st))) return r;
        HIP_TRY(hipMemcpyAsync(acc_out, d_out, s5gpu_pileup_bytes(K), hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        return S5GPU_OK;
    };
    const int rc = fetch();
    if (d_cls) (void)hipFree(d_cls);
    if (d_out) (void)hipFree(d_out);
    if (h->d_acc) (void)hipFree(h->d_acc);                                 // whatever the fold did: the handle ends here
    delete h;
    return rc;
}

extern "C" size_t s5gpu_pileup_long_work_bytes(uint32_t n, uint64_t total_rows) {
    if (total_rows > pilek::LONG_ROWS_MAX) return 0;
    return (size_t)pilek::long_work(n, total_rows).bytes;
}

int pilek::accum_long_checked(const char *who, const PileLongArgs &A, size_t work_bytes, void *hist, bool hist_call, hipStream_t st) {
    if (!hist_call && !acc_ok(who, A.acc, A.R)) return S5GPU_ERR_ARG;
    if (hist_call || hist) {
        if (A.R == 0 || A.R > HIST_RMAX) { s5gpu_set_error("%s: a histogram of %u columns (1 .. 2^22)", who, A.R); return S5GPU_ERR_ARG; }
        if (!hist || ((uintptr_t)hist & 15u)) { s5gpu_set_error("%s: NULL or misaligned hist (16 bytes)", who); return S5GPU_ERR_ARG; }
    }
    if (A.acc && !A.ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    bool go;
    const int rc = long_layout_check(who, A, work_bytes, &go);
    return rc || !go ? rc : launch_pileup_long(A, hist, st);
}

int pilek::long_layout_check(const char *who, const PileLongArgs &A, size_t work_bytes, bool *go) {
    *go = false;
    if (A.total_rows > LONG_ROWS_MAX) { s5gpu_set_error("%s: %llu rows in all (at most 2^40)", who, (unsigned long long)A.total_rows); return S5GPU_ERR_ARG; }
    if (A.n == 0) return S5GPU_OK;
    if (!A.first || !A.qlen || !A.status || !A.work || (A.total_rows && (!A.queries || !A.lo || !A.hi))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)A.queries & 1u) || ((uintptr_t)A.first & 7u) || ((uintptr_t)A.qlen & 3u) || ((uintptr_t)A.ref & 1u) || ((uintptr_t)A.lo & 3u) ||
        ((uintptr_t)A.hi & 3u) || ((uintptr_t)A.status & 3u) || ((uintptr_t)A.events & 15u) || ((uintptr_t)A.work & 15u)) {
        s5gpu_set_error("%s: misaligned argument (first: 8 bytes; events, work: 16)", who);
        return S5GPU_ERR_ARG;
    }
    const uint64_t need = long_work(A.n, A.total_rows).bytes;
    if ((uint64_t)work_bytes < need) {
        s5gpu_set_error("%s: a work area of %zu bytes, %llu are needed", who, work_bytes, (unsigned long long)need);
        return S5GPU_ERR_NOMEM;
    }
    *go = true;
    return S5GPU_OK;
}

extern "C" int s5gpu_pileup_accum_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, const int16_t *ref,
                                           uint32_t R, const int32_t *lo, const int32_t *hi, const int32_t *status, const s5gpu_event_t *events, uint32_t ev_skip,
                                           void *work, size_t work_bytes, void *acc, void *stream) {
    const char *who = "s5gpu_pileup_accum_long_dev";
    pilek::PileLongArgs A;
    A.n = n; A.queries = queries; A.first = first; A.qlen = qlen; A.total_rows = total_rows; A.ref = ref; A.R = R; A.lo = lo; A.hi = hi; A.status = status;
    A.events = events; A.ev_skip = events ? ev_skip : 0u; A.work = work; A.acc = acc;
    return pilek::accum_long_checked(who, A, work_bytes, nullptr, false, (hipStream_t)stream);
}

int pilek::whole_open_check(const char *who, const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, const int16_t *ref_host,
                            uint32_t R) {
    if (dtwk::map_front_check(who, 0, nullptr, nullptr, S5GPU_REC_NONE, S5GPU_SIG_NONE, ep, mp, ref_host, R, true)) return S5GPU_ERR_ARG;
    if (bandk::check_band_params(who, bp) || bandk::check_band_agrees(who, mp, bp)) return S5GPU_ERR_ARG;
    if (R > RMAX) { s5gpu_set_error("%s: a table of %u columns (1 .. 2^26)", who, R); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

extern "C" void *s5gpu_pileup_open_whole(const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, size_t scratch_max,
                                         const int16_t *ref_host, uint32_t R) {
    const char *who = "s5gpu_pileup_open_whole";
    if (pilek::whole_open_check(who, ep, mp, bp, ref_host, R)) return nullptr;
    if (s5host::n_devices() == 0) { s5gpu_set_error("%s: no device", who); return nullptr; }
    Handle *h = new Handle;
    h->whole = true; h->c.ep = *ep; h->c.mp = *mp; h->c.mp.want_start = 1; h->c.bp = *bp; h->c.scratch_max = scratch_max;
    h->c.ref.assign(ref_host, ref_host + R);
    h->d_acc = s5host::acc_open(who, s5gpu_pileup_bytes(R), [R](void *acc, hipStream_t st) { return pilek::launch_reset(acc, R, st); });
    if (!h->d_acc) { delete h; return nullptr; }
    return h;
}

int pilek::add_batch_whole(const char *who, const WholeChain &W, void *d_acc, void *d_hist, const SiteSink *sites, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method,
                           int sig_method, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out) {
    const uint32_t R = (uint32_t)W.ref.size();
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, &W.ep, &W.mp, W.ref.data(), R, true))) return rc;
    if (n == 0) return S5GPU_OK;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, &W.ep, &W.mp, W.ref.data(), R, F))) return rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m;
    bandk::ExtTail E;
    const uint8_t *hb = nullptr, *hrows = nullptr;
    if (m) {
        // the chain of s5gpu_extend_batch; its scratch serves as the work area afterwards (the stream orders them)
        const size_t work_bytes = (size_t)long_work(m, F.total).bytes;
        uint64_t room = 0;
        if ((rc = bandk::extend_tail(who, F, &W.mp, &W.bp, W.scratch_max, R, false, false, ~(size_t)0, work_bytes, &room, E, W.refine ? &W.rp : nullptr))) return rc;
        uint8_t *dg = (uint8_t *)c->d_gather.p;
        const size_t h_rrows = up(E.o_lo + 4ull * m, 16);                  // (refined: the rows of the rounds, behind the statuses)
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, E.o_lo, hipMemcpyDeviceToHost, c->st));
        if (W.refine) HIP_TRY(hipMemcpyAsync((uint8_t *)c->h_out.p + h_rrows, dg + E.r_rows, 32ull * m, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        // a read's status is its result row's, which the host has to complete for the reads that were passed over: up again, over the long
        // queries' statuses, which have served
        hb = (const uint8_t *)c->h_out.p;
        int32_t *h_st = (int32_t *)((uint8_t *)c->h_out.p + E.o_lo);
        hrows = W.refine ? hb + h_rrows : hb;
        for (uint32_t k = 0; k < m; k++) h_st[k] = E.too_big[k] ? S5GPU_STATUS_PATH_WIDE : ((const s5gpu_ext_row_t *)hrows)[k].status;
        HIP_TRY(hipMemcpyAsync(dg + E.o_st, h_st, 4ull * m, hipMemcpyHostToDevice, c->st));
        PileLongArgs A;
        A.n = m; A.queries = (const int16_t *)(dg + E.o_q); A.first = F.d_first; A.qlen = (const uint32_t *)(dg + E.o_ql); A.total_rows = F.total; A.ref = F.d_ref;
        A.R = R; A.lo = (const int32_t *)(dg + E.o_lo); A.hi = (const int32_t *)(dg + E.o_hi); A.status = (const int32_t *)(dg + E.o_st); A.events = F.d_rows;
        A.ev_skip = W.bp.skip; A.work = c->d_scan.p; A.acc = d_acc;
        if (W.refine) { A.queries = (const int16_t *)(dg + E.r_q); A.lo = (const int32_t *)(dg + E.r_lo); A.hi = (const int32_t *)(dg + E.r_hi); }
        if ((d_acc || d_hist) && (rc = accum_long_checked(who, A, work_bytes, d_hist, d_acc == nullptr, c->st))) return rc;
        if (sites && (rc = site_sink_reads(A, work_bytes, *sites, F, n, c->st))) return rc;
    }
    if (sites && (rc = site_sink_rest(*sites, F, n, R, c->st))) return rc;
    if (d_acc && (rc = launch_add_skipped(d_acc, n - m, c->st))) return rc;   // the records that were dropped
    if (d_hist && (rc = launch_hist_add_skipped(d_hist, n - m, c->st))) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));                                  // the next holder of this context overwrites the batch
    dtwk::scatter_rows(F, n, hb ? (const s5gpu_map_row_t *)(hb + E.o_map) : nullptr, nullptr, map_rows_out);
    std::vector<s5gpu_ext_row_t> own;
    if (!ext_rows_out) { own.resize(n); ext_rows_out = own.data(); }      // (the statuses come from the rows)
    bandk::scatter_ext_rows(F, n, E, hrows, ext_rows_out);
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; it counts in reads_skipped)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

int pilek::whole_set_refine(const char *who, WholeChain &W, const s5gpu_refine_params_t *rp) {
    if (W.started) { s5gpu_set_error("%s: the handle has added a batch already", who); return S5GPU_ERR_ARG; }
    if (rp && refk::check_refine_params(who, rp)) return S5GPU_ERR_ARG;
    W.refine = rp != nullptr;
    if (rp) W.rp = *rp;
    return S5GPU_OK;
}

extern "C" int s5gpu_pileup_set_refine(void *handle, const s5gpu_refine_params_t *rp) {
    const char *who = "s5gpu_pileup_set_refine";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!h->whole) { s5gpu_set_error("%s: the handle is one of s5gpu_pileup_open", who); return S5GPU_ERR_ARG; }
    return pilek::whole_set_refine(who, h->c, rp);
}

extern "C" int s5gpu_pileup_add_batch_whole(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                            s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out) {
    const char *who = "s5gpu_pileup_add_batch_whole";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!h->whole) { s5gpu_set_error("%s: the handle is one of s5gpu_pileup_open", who); return S5GPU_ERR_ARG; }
    h->c.started = true;
    return pilek::add_batch_whole(who, h->c, h->d_acc, nullptr, nullptr, n, rec, rec_len, rec_method, sig_method, map_rows_out, ext_rows_out, status_out);
}
