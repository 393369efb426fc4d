// pileup_api.hip — host side of the pileup calls (include/slow5gpu.h, "pileup"; docs/codecs.md §4.18): the accumulator's size, argument
// checks and launches of the two device entry points, and the per-file handle: s5gpu_pileup_add_batch runs the chain of s5gpu_align_batch
// (the front of dtw_host.h -> sDTW with the start -> the paths -> the query's event rows gathered) and adds the batch to the handle's
// accumulator with k_pileup; the rows and statuses are all that comes back.  s5gpu_pileup_close makes the one download of the table.
#include "dtw_host.h"
#include "pileup_dev.h"

namespace {

struct Handle {
    void *d_acc = nullptr;
    s5gpu_event_params_t ep;
    s5gpu_map_params_t mp;
    uint32_t wmax = 0;
    std::vector<int16_t> ref;
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
    h->ep = *ep; h->mp = *mp; h->mp.want_start = 1; h->wmax = wmax;
    h->ref.assign(ref_host, ref_host + R);
    h->d_acc = s5host::acc_open(who, s5gpu_pileup_bytes(R), [R](void *acc, hipStream_t st) { return pilek::launch_reset(acc, R, st); });
    if (!h->d_acc) { delete h; return nullptr; }
    return h;
}

extern "C" int s5gpu_pileup_add_batch(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                      s5gpu_map_row_t *rows_out, int32_t *status_out) {
    const char *who = "s5gpu_pileup_add_batch";
    Handle *h = (Handle *)handle;
    if (!h || !h->d_acc) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    const uint32_t R = (uint32_t)h->ref.size(), qmax = h->mp.qmax;
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, &h->ep, &h->mp, h->ref.data(), R, true))) return rc;
    if (n == 0) return S5GPU_OK;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, &h->ep, &h->mp, h->ref.data(), R, F))) return rc;
    Ctx *c = F.hold.c;
    // in c->d_gather: the rows and the path statuses, which come back, and lo, hi and the events, which do not
    const dtwk::PathTail T = dtwk::path_layout(F.m, qmax, true);
    if (F.m) {
        if ((rc = dtwk::path_tail(F, &h->mp, h->wmax, R, true, T, T.o_lo))) return rc;
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
    const int rc = s5host::acc_close(h->d_acc, s5gpu_pileup_bytes((uint32_t)h->ref.size()), acc_out, true);
    delete h;
    return rc;
}
