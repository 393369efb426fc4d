// pileup_api.hip — host side of the pileup calls (include/slow5gpu.h, "pileup"; docs/codecs.md §4.18): the accumulator's size, argument
// checks and launches of the two device entry points, and the per-file handle: s5gpu_pileup_add_batch runs the chain of s5gpu_align_batch
// (the front of dtw_host.h -> sDTW with the start -> the paths -> the query's event rows gathered) and adds the batch to the handle's
// accumulator with k_pileup; the rows and statuses are all that comes back.  s5gpu_pileup_close makes the one download of the table.
#include "dtw_host.h"
#include "pileup_dev.h"

namespace {

constexpr size_t PILE_SCRATCH_MAX = (size_t)256 << 20;                     // the scratch of the paths at most, as s5gpu_align_batch

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
    if (wmax == 0 || wmax > dtwk::WMAX) { s5gpu_set_error("%s: wmax %u (1 .. %u)", who, wmax, dtwk::WMAX); return nullptr; }
    if (R > pilek::RMAX) { s5gpu_set_error("%s: a table of %u columns (1 .. 2^26)", who, R); return nullptr; }
    const size_t slot = s5gpu_sdtw_path_slot_bytes(mp->qmax, wmax);
    if (slot > PILE_SCRATCH_MAX) { s5gpu_set_error("%s: a read needs %zu bytes of scratch, above the %zu of this call", who, slot, PILE_SCRATCH_MAX); return nullptr; }
    if (s5host::n_devices() == 0) { s5gpu_set_error("%s: no device", who); return nullptr; }
    s5host::CtxHold hold;
    if (hold.acquire(0)) return nullptr;
    Ctx *c = hold.c;
    Handle *h = new Handle;
    h->ep = *ep; h->mp = *mp; h->mp.want_start = 1; h->wmax = wmax;
    h->ref.assign(ref_host, ref_host + R);
    hipError_t e = hipMalloc(&h->d_acc, s5gpu_pileup_bytes(R));
    if (e != hipSuccess) {
        s5gpu_set_error("%s: allocation of the accumulator failed: %s", who, hipGetErrorString(e));
        delete h;
        return nullptr;
    }
    if (pilek::launch_reset(h->d_acc, R, c->st) != S5GPU_OK || hipStreamSynchronize(c->st) != hipSuccess) {
        (void)hipFree(h->d_acc);
        delete h;
        return nullptr;
    }
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
    const size_t slot = s5gpu_sdtw_path_slot_bytes(qmax, h->wmax);
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, &h->ep, &h->mp, h->ref.data(), R, F))) return rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m;
    const s5gpu_map_row_t empty = {dtwk::NO_COST, 0, -1, -1};
    if (rows_out)
        for (uint32_t i = 0; i < n; i++) rows_out[i] = empty;             // what a record that was dropped keeps
    if (m) {
        // in c->d_gather: the rows [m] and the path statuses [m], which come back, and lo, hi [m, qmax] and the events [m, qmax], which do not
        const size_t row_i = (size_t)qmax;
        const size_t o_pst = up(16ull * m, 16), o_lo = o_pst + up(4ull * m, 16), o_hi = o_lo + up(4ull * m * row_i, 16), o_ev = o_hi + up(4ull * m * row_i, 16),
                     bytes = o_ev + 16ull * m * row_i, back = o_lo;
        const size_t scratch = slot * m < PILE_SCRATCH_MAX ? slot * m : PILE_SCRATCH_MAX / slot * slot;
        if ((rc = c->d_gather.reserve(bytes + 64)) || (rc = c->d_scan.reserve(scratch + 64)) || (rc = c->h_out.reserve(back + 64))) return rc;
        uint8_t *dg = (uint8_t *)c->d_gather.p;
        s5gpu_map_row_t *d_out = (s5gpu_map_row_t *)dg;
        int32_t *d_pst = (int32_t *)(dg + o_pst), *d_lo = (int32_t *)(dg + o_lo), *d_hi = (int32_t *)(dg + o_hi);
        s5gpu_event_t *d_ev = (s5gpu_event_t *)(dg + o_ev);
        if ((rc = dtwk::launch_sdtw(m, F.d_q, qmax, F.d_ql, F.d_ref, R, true, d_out, c->st)) ||
            (rc = s5gpu_sdtw_path_dev(m, F.d_q, qmax, F.d_ql, F.d_ref, R, d_out, h->wmax, c->d_scan.p, scratch, d_lo, d_hi, d_pst, c->st)) ||
            (rc = dtwk::launch_event_gather(m, F.d_rows, F.d_first, F.d_ql, h->mp.skip, qmax, d_ev, c->st)) ||
            (rc = s5gpu_pileup_accum_dev(m, F.d_q, qmax, F.d_ql, F.d_ref, R, d_lo, d_hi, d_pst, d_ev, h->d_acc, c->st)))
            return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, back, hipMemcpyDeviceToHost, c->st));
    }
    if ((rc = pilek::launch_add_skipped(h->d_acc, n - m, c->st))) return rc;   // the records that were dropped
    HIP_TRY(hipStreamSynchronize(c->st));                                  // the next holder of this context overwrites the batch
    if (m) {
        const uint8_t *hb = (const uint8_t *)c->h_out.p;
        const s5gpu_map_row_t *hr = (const s5gpu_map_row_t *)hb;
        const int32_t *h_pst = (const int32_t *)(hb + up(16ull * m, 16));
        for (uint32_t k = 0; k < m; k++) {
            const size_t i = F.cur[k];
            if (rows_out) rows_out[i] = hr[k];
            if (F.status[i] == 0) F.status[i] = hr[k].qlen == 0 ? S5GPU_STATUS_QUERY_SHORT : h_pst[k];
        }
    }
    if (status_out) memcpy(status_out, F.status.data(), sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0; it counts in reads_skipped)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

extern "C" int s5gpu_pileup_close(void *handle, void *acc_out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    auto fetch = [&]() -> int {
        s5host::CtxHold hold;
        int r;
        if ((r = hold.acquire(0))) return r;
        Ctx *c = hold.c;
        HIP_TRY(hipMemcpyAsync(acc_out, h->d_acc, s5gpu_pileup_bytes((uint32_t)h->ref.size()), hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        return S5GPU_OK;
    };
    const int rc = h->d_acc && acc_out ? fetch() : S5GPU_OK;
    if (h->d_acc) (void)hipFree(h->d_acc);                                 // whatever the download did: the handle ends here
    delete h;
    return rc;
}
