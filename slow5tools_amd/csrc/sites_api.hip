// sites_api.hip — host side of the sites calls (include/slow5gpu.h, "sites"; docs/codecs.md §4.25): argument checks and launches of the two
// device entry points, what a batch of a whole-read handle leaves of its sites (the sink of pilek::add_batch_whole), and the per-file handle:
// s5gpu_sites_add_control is s5gpu_pileup_add_batch_whole into the control histogram alone, s5gpu_sites_add_batch the same chain into the
// site matrix and its scores.
#include "pileup_host.h"

namespace {

struct Handle {
    pilek::WholeChain c;
    uint32_t *d_sites = nullptr;
    uint32_t M = 0;
    void *d_hist = nullptr;
    int32_t q0 = 0;
    uint32_t shift = 0;
};

// a device allocation that ends with its scope
struct DevMem {
    void *p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
};

bool matrix_ok(const char *who, uint32_t n, uint32_t M) {
    if (M == 0 || M > pilek::SITES_MAX) { s5gpu_set_error("%s: %u sites (1 .. 65536)", who, M); return false; }
    if ((uint64_t)M * n > pilek::SITE_CELLS_MAX) { s5gpu_set_error("%s: %u sites of %u reads (at most 2^27 entries)", who, M, n); return false; }
    return true;
}

void free_handle(Handle *h) {
    if (h->d_sites) (void)hipFree(h->d_sites);
    if (h->d_hist) (void)hipFree(h->d_hist);
    delete h;
}

}  // namespace

extern "C" int s5gpu_site_cells_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, uint32_t R,
                                         const int32_t *lo, const int32_t *hi, const int32_t *status, const uint32_t *sites_dev, uint32_t M, void *work,
                                         size_t work_bytes, s5gpu_site_cell_t *cells_out, uint32_t *verdict_out, void *stream) {
    const char *who = "s5gpu_site_cells_long_dev";
    pilek::PileLongArgs A;
    A.n = n; A.queries = queries; A.first = first; A.qlen = qlen; A.total_rows = total_rows; A.ref = nullptr; A.R = R; A.lo = lo; A.hi = hi; A.status = status;
    A.events = nullptr; A.ev_skip = 0u; A.work = work; A.acc = nullptr;
    if (R == 0 || R > pilek::HIST_RMAX) { s5gpu_set_error("%s: %u columns (1 .. 2^22)", who, R); return S5GPU_ERR_ARG; }
    if (!matrix_ok(who, n, M)) return S5GPU_ERR_ARG;
    if (!sites_dev || ((uintptr_t)sites_dev & 3u) || !cells_out || ((uintptr_t)cells_out & 15u) || ((uintptr_t)verdict_out & 3u)) {
        s5gpu_set_error("%s: NULL or misaligned sites_dev, cells_out (16 bytes) or verdict_out", who);
        return S5GPU_ERR_ARG;
    }
    bool go;
    const int rc = pilek::long_layout_check(who, A, work_bytes, &go);
    return rc || !go ? rc : pilek::launch_site_cells(A, sites_dev, M, cells_out, verdict_out, (hipStream_t)stream);
}

extern "C" int s5gpu_site_score_dev(const s5gpu_site_cell_t *cells, uint32_t n, const uint32_t *sites_dev, uint32_t M, const void *hist, uint32_t R,
                                    s5gpu_site_score_t *out, void *stream) {
    const char *who = "s5gpu_site_score_dev";
    if (R == 0 || R > pilek::HIST_RMAX) { s5gpu_set_error("%s: a histogram of %u columns (1 .. 2^22)", who, R); return S5GPU_ERR_ARG; }
    if (!matrix_ok(who, n, M)) return S5GPU_ERR_ARG;
    if (!cells || !sites_dev || !hist || !out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)cells & 15u) || ((uintptr_t)sites_dev & 3u) || ((uintptr_t)hist & 15u) || ((uintptr_t)out & 15u)) {
        s5gpu_set_error("%s: misaligned argument (cells, hist, out: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    return pilek::launch_site_score(cells, n, sites_dev, M, hist, R, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- the sink of a batch

int pilek::site_sink_reads(const PileLongArgs &A, size_t work_bytes, const SiteSink &S, const dtwk::MapFront &F, uint32_t n, hipStream_t st) {
    const uint32_t m = A.n, M = S.M;
    const size_t entries = (size_t)M * m;
    DevMem d_cells, d_scores;
    std::vector<s5gpu_site_cell_t> h_cells(entries);
    std::vector<s5gpu_site_score_t> h_scores(S.scores_out ? entries : 0);
    HIP_TRY(hipMalloc(&d_cells.p, 16 * entries));
    int rc;
    if ((rc = s5gpu_site_cells_long_dev(m, A.queries, A.first, A.qlen, A.total_rows, A.R, A.lo, A.hi, A.status, S.d_sites, M, A.work, work_bytes,
                                        (s5gpu_site_cell_t *)d_cells.p, nullptr, st)))
        return rc;
    HIP_TRY(hipMemcpyAsync(h_cells.data(), d_cells.p, 16 * entries, hipMemcpyDeviceToHost, st));
    if (S.scores_out) {
        HIP_TRY(hipMalloc(&d_scores.p, 16 * entries));
        if ((rc = s5gpu_site_score_dev((const s5gpu_site_cell_t *)d_cells.p, m, S.d_sites, M, S.d_control, A.R, (s5gpu_site_score_t *)d_scores.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(h_scores.data(), d_scores.p, 16 * entries, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t t = 0; t < M; t++)
        for (uint32_t k = 0; k < m; k++) {
            const size_t to = (size_t)t * n + F.cur[k], from = (size_t)t * m + k;
            S.cells_out[to] = h_cells[from];
            if (S.scores_out) S.scores_out[to] = h_scores[from];
        }
    return S5GPU_OK;
}

// the records that were dropped: the empty entry, and the row k_site_score gives one at each site (a matrix of M sites and one read)
int pilek::site_sink_rest(const SiteSink &S, const dtwk::MapFront &F, uint32_t n, uint32_t R, hipStream_t st) {
    const uint32_t m = F.m, M = S.M;
    if (m == n) return S5GPU_OK;
    std::vector<uint8_t> there(n, 0);
    for (uint32_t k = 0; k < m; k++) there[F.cur[k]] = 1;
    const s5gpu_site_cell_t empty = {0, 0u, SITE_ROW_NONE};
    std::vector<s5gpu_site_cell_t> h_cells(M, empty);
    std::vector<s5gpu_site_score_t> h_scores(S.scores_out ? M : 0);
    if (S.scores_out) {
        DevMem d_cells, d_scores;
        HIP_TRY(hipMalloc(&d_cells.p, 16 * (size_t)M));
        HIP_TRY(hipMalloc(&d_scores.p, 16 * (size_t)M));
        HIP_TRY(hipMemcpyAsync(d_cells.p, h_cells.data(), 16 * (size_t)M, hipMemcpyHostToDevice, st));
        int rc;
        if ((rc = s5gpu_site_score_dev((const s5gpu_site_cell_t *)d_cells.p, 1u, S.d_sites, M, S.d_control, R, (s5gpu_site_score_t *)d_scores.p, st))) return rc;
        HIP_TRY(hipMemcpyAsync(h_scores.data(), d_scores.p, 16 * (size_t)M, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    for (uint32_t t = 0; t < M; t++)
        for (uint32_t i = 0; i < n; i++) {
            if (there[i]) continue;
            S.cells_out[(size_t)t * n + i] = empty;
            if (S.scores_out) S.scores_out[(size_t)t * n + i] = h_scores[t];
        }
    return S5GPU_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the handle

extern "C" void *s5gpu_sites_open(const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, size_t scratch_max,
                                  const int16_t *ref_host, uint32_t R, const uint32_t *sites_host, uint32_t M, int32_t q0, uint32_t shift) {
    const char *who = "s5gpu_sites_open";
    if (pilek::whole_open_check(who, ep, mp, bp, ref_host, R)) return nullptr;
    if (R > pilek::HIST_RMAX) { s5gpu_set_error("%s: a histogram of %u columns (1 .. 2^22)", who, R); return nullptr; }
    if (q0 < -32768 || q0 > 32767 || shift > pilek::HIST_SHIFT_MAX) { s5gpu_set_error("%s: q0 %d (-32768 .. 32767), shift %u (0 .. 10)", who, q0, shift); return nullptr; }
    if (!sites_host || !matrix_ok(who, 0, M)) { if (!sites_host) s5gpu_set_error("%s: NULL site list", who); return nullptr; }
    for (uint32_t t = 0; t < M; t++)
        if (sites_host[t] >= R || (t && sites_host[t] <= sites_host[t - 1])) {
            s5gpu_set_error("%s: site %u is column %u: the list is strictly increasing and below R = %u", who, t, sites_host[t], R);
            return nullptr;
        }
    if (s5host::n_devices() == 0) { s5gpu_set_error("%s: no device", who); return nullptr; }
    Handle *h = new Handle;
    h->c.ep = *ep; h->c.mp = *mp; h->c.mp.want_start = 1; h->c.bp = *bp; h->c.scratch_max = scratch_max;
    h->c.ref.assign(ref_host, ref_host + R);
    h->M = M; h->q0 = q0; h->shift = shift;
    h->d_hist = s5host::acc_open(who, s5gpu_pile_hist_bytes(R), [=](void *hist, hipStream_t st) { return pilek::launch_hist_reset(hist, R, q0, shift, st); });
    // (the list goes up as an accumulator's first contents)
    h->d_sites = (uint32_t *)s5host::acc_open(who, 4 * (size_t)M, [=](void *p, hipStream_t st) -> int {
        HIP_TRY(hipMemcpyAsync(p, sites_host, 4 * (size_t)M, hipMemcpyHostToDevice, st));
        return S5GPU_OK;
    });
    if (!h->d_hist || !h->d_sites) { free_handle(h); return nullptr; }
    return h;
}

extern "C" int s5gpu_sites_set_refine(void *handle, const s5gpu_refine_params_t *rp) {
    const char *who = "s5gpu_sites_set_refine";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    return pilek::whole_set_refine(who, h->c, rp);
}

extern "C" int s5gpu_sites_add_control(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, int32_t *status_out) {
    const char *who = "s5gpu_sites_add_control";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    h->c.started = true;
    return pilek::add_batch_whole(who, h->c, nullptr, h->d_hist, nullptr, n, rec, rec_len, rec_method, sig_method, nullptr, nullptr, status_out);
}

extern "C" int s5gpu_sites_set_control(void *handle, const void *hist_host) {
    const char *who = "s5gpu_sites_set_control";
    Handle *h = (Handle *)handle;
    if (!h || !hist_host) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    s5gpu_pile_hist_head_t head;
    memcpy(&head, hist_host, sizeof head);
    const uint32_t R = (uint32_t)h->c.ref.size();
    if (head.R != R || head.q0 != h->q0 || head.shift != h->shift || head.bins != pilek::HIST_BINS) {
        s5gpu_set_error("%s: a histogram of R %u, q0 %d, shift %u, %u bins; the handle's are %u, %d, %u, 64", who, head.R, head.q0, head.shift, head.bins, R, h->q0, h->shift);
        return S5GPU_ERR_ARG;
    }
    s5host::CtxHold hold;
    int r;
    if ((r = hold.acquire(0))) return r;
    Ctx *c = hold.c;
    HIP_TRY(hipMemcpyAsync(h->d_hist, hist_host, s5gpu_pile_hist_bytes(R), hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return S5GPU_OK;
}

extern "C" int s5gpu_sites_add_batch(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                     s5gpu_ext_row_t *ext_rows_out, s5gpu_site_cell_t *cells_out, s5gpu_site_score_t *scores_out, int32_t *status_out) {
    const char *who = "s5gpu_sites_add_batch";
    Handle *h = (Handle *)handle;
    if (!h) { s5gpu_set_error("%s: NULL handle", who); return S5GPU_ERR_ARG; }
    if (!matrix_ok(who, n, h->M)) return S5GPU_ERR_ARG;
    if (n && !cells_out) { s5gpu_set_error("%s: NULL cells_out", who); return S5GPU_ERR_ARG; }
    h->c.started = true;
    const pilek::SiteSink S = {h->d_sites, h->M, h->d_hist, cells_out, scores_out};
    return pilek::add_batch_whole(who, h->c, nullptr, nullptr, &S, n, rec, rec_len, rec_method, sig_method, nullptr, ext_rows_out, status_out);
}

extern "C" int s5gpu_sites_close(void *handle, void *hist_out) {
    Handle *h = (Handle *)handle;
    if (!h) return S5GPU_OK;
    const int rc = s5host::acc_close(h->d_hist, s5gpu_pile_hist_bytes((uint32_t)h->c.ref.size()), hist_out, true);
    h->d_hist = nullptr;                                                   // (freed by the close, whatever the download did)
    free_handle(h);
    return rc;
}
