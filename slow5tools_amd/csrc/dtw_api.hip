// dtw_api.hip — host side of the map calls (include/slow5gpu.h, "map"): the quantiser on the host, argument checks and the launches of
// the device entry points, and s5gpu_map_batch: upload -> decode -> event passes -> queries -> sDTW -> 16 bytes per read come back
// (and, before the fill pass, the 8 bytes of the event total: the host has to know the room the rows need).
// s5gpu_sdtw2_dev and s5gpu_map2_batch are the same with the second-best hit beside each row (k_sdtw2, docs/codecs.md §4.19).
// Neither the decoded signals nor the events leave the device.  The chain up to the queries is map_front (dtw_host.h), which
// s5gpu_align_batch (dtw_path_api.hip) and s5gpu_pileup_add_batch (pileup_api.hip) run too.
#include <math.h>

#include "dtw_host.h"
#include "event_host.h"

namespace {

int check_quant(const char *who, double scale, int32_t clip) {
    if (!isfinite(scale) || !(scale > 0.0)) { s5gpu_set_error("%s: scale %g (finite, > 0)", who, scale); return S5GPU_ERR_ARG; }
    if (clip < 1 || clip > 32767) { s5gpu_set_error("%s: clip %d (1 .. 32767)", who, clip); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

int check_params(const char *who, const s5gpu_map_params_t *p) {
    if (!p) { s5gpu_set_error("%s: NULL parameters", who); return S5GPU_ERR_ARG; }
    if (p->qmax == 0 || p->qmax > dtwk::QMAX) { s5gpu_set_error("%s: qmax %u (1 .. %u)", who, p->qmax, dtwk::QMAX); return S5GPU_ERR_ARG; }
    if (p->qmin == 0 || p->qmin > p->qmax) { s5gpu_set_error("%s: qmin %u (1 .. qmax = %u)", who, p->qmin, p->qmax); return S5GPU_ERR_ARG; }
    return check_quant(who, p->scale, p->clip);
}

dtwk::QueryArgs args_of(const s5gpu_event_t *rows, const uint64_t *first, const int32_t *ev_status, const s5gpu_map_params_t *p, int16_t *queries,
                        uint32_t *qlen, int32_t *status) {
    dtwk::QueryArgs A;
    A.rows = rows; A.first = first; A.ev_status = ev_status;
    A.skip = p->skip; A.qmax = p->qmax; A.qmin = p->qmin; A.scale = p->scale; A.clip = p->clip;
    A.queries = queries; A.qlen = qlen; A.status = status;
    return A;
}

}  // namespace

int dtwk::check_ref(const char *who, uint32_t R) {
    if (R == 0 || R > 0x7FFFFFFFu) { s5gpu_set_error("%s: a reference of %u values (1 .. 2^31 - 1)", who, R); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

extern "C" int s5gpu_quantise_host(const float *m, size_t L, double scale, int32_t clip, int16_t *q) {
    const char *who = "s5gpu_quantise_host";
    int rc;
    if ((rc = check_quant(who, scale, clip))) return rc;
    if (L == 0) return S5GPU_OK;
    if (!m || !q) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    dtwk::quant_row(m, 1, L, scale, clip, q);
    return S5GPU_OK;
}

extern "C" int s5gpu_event_queries_dev(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const int32_t *ev_status,
                                       const s5gpu_map_params_t *p, int16_t *queries, uint32_t *qlen, int32_t *status, void *stream) {
    const char *who = "s5gpu_event_queries_dev";
    int rc;
    if ((rc = check_params(who, p))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!first || !queries || !qlen || !status) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }   // (rows: NULL when no read has one)
    if (((uintptr_t)rows & 15u) || ((uintptr_t)first & 7u) || ((uintptr_t)ev_status & 3u) || ((uintptr_t)queries & 1u) || ((uintptr_t)qlen & 3u) ||
        ((uintptr_t)status & 3u)) {
        s5gpu_set_error("%s: misaligned argument (rows: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    return dtwk::launch_queries(n, args_of(rows, first, ev_status, p, queries, qlen, status), (hipStream_t)stream);
}

extern "C" int s5gpu_sdtw_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, int want_start,
                              s5gpu_map_row_t *out_rows, void *stream) {
    const char *who = "s5gpu_sdtw_dev";
    int rc;
    if (qpitch == 0 || qpitch > dtwk::QMAX) { s5gpu_set_error("%s: a pitch of %u values (1 .. %u)", who, qpitch, dtwk::QMAX); return S5GPU_ERR_ARG; }
    if ((rc = dtwk::check_ref(who, R))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !out_rows) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)queries & 1u) || ((uintptr_t)qlen & 3u) || ((uintptr_t)ref & 1u) || ((uintptr_t)out_rows & 15u)) {
        s5gpu_set_error("%s: misaligned argument (out_rows: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    return dtwk::launch_sdtw(n, queries, qpitch, qlen, ref, R, want_start != 0, out_rows, (hipStream_t)stream);
}

static int check_bshift(const char *who, uint32_t bshift) {
    if (bshift < 6 || bshift > 30) { s5gpu_set_error("%s: a block shift of %u (6 .. 30)", who, bshift); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

extern "C" int s5gpu_sdtw2_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, int want_start,
                               uint32_t bshift, s5gpu_map_row_t *out_rows, s5gpu_map_second_t *out_second, void *stream) {
    const char *who = "s5gpu_sdtw2_dev";
    int rc;
    if (qpitch == 0 || qpitch > dtwk::QMAX) { s5gpu_set_error("%s: a pitch of %u values (1 .. %u)", who, qpitch, dtwk::QMAX); return S5GPU_ERR_ARG; }
    if ((rc = dtwk::check_ref(who, R)) || (rc = check_bshift(who, bshift))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (!out_second || ((uintptr_t)out_second & 15u)) { s5gpu_set_error("%s: out_second is NULL or not 16-byte aligned", who); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !out_rows) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (((uintptr_t)queries & 1u) || ((uintptr_t)qlen & 3u) || ((uintptr_t)ref & 1u) || ((uintptr_t)out_rows & 15u)) {
        s5gpu_set_error("%s: misaligned argument (out_rows: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    return dtwk::launch_sdtw2(n, queries, qpitch, qlen, ref, R, want_start != 0, bshift, out_rows, out_second, (hipStream_t)stream);
}

int dtwk::map_front_check(const char *who, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                          const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, bool outputs) {
    int rc;
    if ((rc = evk::check_params(who, ep, S5GPU_NORM_RAW)) || (rc = check_params(who, mp)) || (rc = check_ref(who, R))) return rc;
    if (!s5rules::methods_ok(rec_method, sig_method)) { s5gpu_set_error("%s: unsupported method", who); return S5GPU_ERR_ARG; }
    if (!ref_host || (n && (!rec || !rec_len || !outputs))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    return s5rules::host_records_ok(who, n, rec, rec_len);
}

int dtwk::map_front(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
                    const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, MapFront &F) {
    int rc;
    if ((rc = F.hold.acquire(0))) return rc;
    Ctx *c = F.hold.c;
    if ((rc = s5host::resident_records(c, n, rec, rec_len, rec_method, sig_method, F))) return rc;
    const uint32_t m = F.m;
    if (m == 0) return S5GPU_OK;
    // on the device: first[m + 1] (u64), the events' counts and statuses [m], qlen[m], the queries' statuses [m], the result rows [m] ...
    const size_t o_cnt = up(8ull * (m + 1), 16), o_est = o_cnt + up(4ull * m, 16), o_ql = o_est + up(4ull * m, 16), o_qst = o_ql + up(4ull * m, 16),
                 o_out = o_qst + up(4ull * m, 16);
    if ((rc = c->d_patch.reserve(o_out + 16ull * m + 64)) || (rc = c->h_out.reserve(16ull * m + 64))) return rc;
    uint8_t *dp = (uint8_t *)c->d_patch.p;
    uint64_t *d_first = (uint64_t *)dp;
    uint32_t *d_cnt = (uint32_t *)(dp + o_cnt), *d_ql = (uint32_t *)(dp + o_ql);
    int32_t *d_est = (int32_t *)(dp + o_est), *d_qst = (int32_t *)(dp + o_qst);
    const sigk::SigRecs S = s5host::resident_sig_recs(c, m);
    uint64_t total = 0;                                                   // the host has to know the room the rows need
    if ((rc = evk::events_count(c, S, ep, S5GPU_NORM_RAW, d_first, d_cnt, d_est, 1, &total))) return rc;
    // ... and the event rows, the query matrix and the reference
    const size_t o_q = up(16ull * total, 16), o_ref = o_q + up(2ull * m * mp->qmax, 16);
    if ((rc = c->d_stream.reserve(o_ref + 2ull * R + 64))) return rc;
    uint8_t *ds = (uint8_t *)c->d_stream.p;
    s5gpu_event_t *d_rows = (s5gpu_event_t *)ds;
    int16_t *d_q = (int16_t *)(ds + o_q), *d_ref = (int16_t *)(ds + o_ref);
    HIP_TRY(hipMemcpyAsync(d_ref, ref_host, 2ull * R, hipMemcpyHostToDevice, c->st));
    if (total && (rc = evk::launch_events(S, evk::args_of(ep, S5GPU_NORM_RAW, d_first, d_cnt, d_rows, d_cnt, d_est), c->st))) return rc;
    if ((rc = dtwk::launch_queries(m, args_of(d_rows, d_first, d_est, mp, d_q, d_ql, d_qst), c->st))) return rc;
    F.d_rows = d_rows; F.d_first = d_first; F.d_q = d_q; F.d_ql = d_ql; F.d_ref = d_ref;
    F.d_out = (s5gpu_map_row_t *)(dp + o_out);
    F.d_est = d_est; F.total = total;
    return S5GPU_OK;
}

extern "C" int s5gpu_map_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                               const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R,
                               s5gpu_map_row_t *rows_out, int32_t *status_out) {
    const char *who = "s5gpu_map_batch";
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, rows_out != nullptr))) return rc;
    if (n == 0) return S5GPU_OK;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, F))) return rc;
    Ctx *c = F.hold.c;
    if (F.m) {
        if ((rc = dtwk::launch_sdtw(F.m, F.d_q, mp->qmax, F.d_ql, F.d_ref, R, mp->want_start != 0, F.d_out, c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, F.d_out, 16ull * F.m, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    dtwk::scatter_rows(F, n, (const s5gpu_map_row_t *)c->h_out.p, nullptr, rows_out);
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its row is empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}

// s5gpu_map_batch through k_sdtw2: the second rows of the m decoded reads are made in c->d_gather (the front leaves it alone) and come back
// behind the rows, in one download
extern "C" int s5gpu_map2_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                const s5gpu_event_params_t *ep, const s5gpu_map_params_t *mp, const int16_t *ref_host, uint32_t R, uint32_t bshift,
                                s5gpu_map_row_t *rows_out, s5gpu_map_second_t *second_out, int32_t *status_out) {
    const char *who = "s5gpu_map2_batch";
    const s5gpu_map_second_t none = {dtwk::NO_COST, -1, 0, 0};
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, rows_out != nullptr && second_out != nullptr)) ||
        (rc = check_bshift(who, bshift)))
        return rc;
    if (n == 0) return S5GPU_OK;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, F))) return rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m;
    const s5gpu_map_second_t *h2 = nullptr;
    if (m) {
        const size_t o2 = up(16ull * m, 16);
        if ((rc = c->d_gather.reserve(32ull * m + 64)) || (rc = c->h_out.reserve(o2 + 16ull * m + 64))) return rc;
        s5gpu_map_row_t *d_rows = (s5gpu_map_row_t *)c->d_gather.p;
        s5gpu_map_second_t *d_second = (s5gpu_map_second_t *)((uint8_t *)c->d_gather.p + o2);
        if ((rc = dtwk::launch_sdtw2(m, F.d_q, mp->qmax, F.d_ql, F.d_ref, R, mp->want_start != 0, bshift, d_rows, d_second, c->st))) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, c->d_gather.p, o2 + 16ull * m, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        h2 = (const s5gpu_map_second_t *)((const uint8_t *)c->h_out.p + o2);
    }
    dtwk::scatter_rows(F, n, (const s5gpu_map_row_t *)c->h_out.p, nullptr, rows_out);
    for (uint32_t i = 0; i < n; i++) second_out[i] = none;
    for (uint32_t k = 0; k < m; k++) second_out[F.cur[k]] = h2[k];
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its rows are empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
