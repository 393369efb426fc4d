// refine_api.hip — host side of the refine calls (include/slow5gpu.h, "refine"; docs/codecs.md §4.20): argument checks and launches of
// s5gpu_path_fit_dev and s5gpu_sdtw_window_dev, the rounds of s5gpu_refine_dev, and s5gpu_refine_batch: the chain of s5gpu_align_batch
// (the front and the path tail of dtw_host.h) -> the rounds -> one download.
#include "refine_host.h"

int refk::check_refine_params(const char *who, const s5gpu_refine_params_t *p) {
    if (!p) { s5gpu_set_error("%s: NULL refine parameters", who); return S5GPU_ERR_ARG; }
    if (!refk::params_ok(*p)) {
        s5gpu_set_error("%s: refine parameters a_min %g a_max %g (finite, 0 < a_min <= a_max) b_max %g (finite, >= 0) clip %d (1 .. 32767) pad %u (0 .. 65535) "
                        "min_cells %u (>= 2) iters %u (1 .. 4)", who, p->a_min, p->a_max, p->b_max, p->clip, p->pad, p->min_cells, p->iters);
        return S5GPU_ERR_ARG;
    }
    return S5GPU_OK;
}

using refk::check_refine_params;

namespace {

int check_shape(const char *who, uint32_t qpitch, uint32_t R, uint32_t wmax, const int16_t *ref) {
    if (qpitch == 0 || qpitch > dtwk::QMAX) { s5gpu_set_error("%s: a pitch of %u values (1 .. %u)", who, qpitch, dtwk::QMAX); return S5GPU_ERR_ARG; }
    int rc;
    if ((rc = dtwk::check_ref(who, R)) || (rc = dtwk::check_wmax(who, wmax))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

bool mis(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

// the places of a trial round in `work`
struct Work { size_t o_rows, o_fit, o_sf, o_sw, o_lo, o_hi, o_q, bytes; };
Work work_layout(uint32_t n, uint32_t qpitch) {
    Work W;
    const uint64_t m = n ? n : 1;
    W.o_rows = 0; W.o_fit = up(16ull * m, 16); W.o_sf = W.o_fit + 64ull * m; W.o_sw = W.o_sf + up(4ull * m, 16); W.o_lo = W.o_sw + up(4ull * m, 16);
    W.o_hi = W.o_lo + up(4ull * m * qpitch, 16); W.o_q = W.o_hi + up(4ull * m * qpitch, 16); W.bytes = W.o_q + up(2ull * m * qpitch, 16);
    return W;
}

// the window launches of n reads, in groups of as many reads as the scratch has slots (the stream orders the groups)
int window_groups(const char *who, uint32_t n, refk::WinArgs A, void *scratch, size_t scratch_bytes, hipStream_t st) {
    const size_t slot = s5gpu_sdtw_path_slot_bytes(A.qpitch, A.wmax);
    if (scratch_bytes < slot) { s5gpu_set_error("%s: a scratch of %zu bytes, a read needs %zu", who, scratch_bytes, slot); return S5GPU_ERR_NOMEM; }
    const size_t fit = scratch_bytes / slot;
    const uint32_t group = fit < n ? (uint32_t)fit : n;
    const refk::WinArgs B = A;
    for (uint32_t b = 0; b < n; b += group) {
        A.queries = B.queries + (size_t)b * B.qpitch; A.qlen = B.qlen + b; A.rows_in = B.rows_in + b; A.gate = B.gate ? B.gate + b : nullptr;
        A.scratch = (uint32_t *)scratch; A.slot_words = dtwk::path_slot_words(B.qpitch, B.wmax);
        A.rows_out = B.rows_out + b; A.lo = B.lo + (size_t)b * B.qpitch; A.hi = B.hi + (size_t)b * B.qpitch; A.status = B.status + b;
        int rc;
        if ((rc = refk::launch_window(n - b < group ? n - b : group, A, st))) return rc;
    }
    return S5GPU_OK;
}

}  // namespace

extern "C" int s5gpu_path_fit_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, const int32_t *lo,
                                  const int32_t *hi, const int32_t *status_in, uint32_t wmax, const s5gpu_refine_params_t *params, s5gpu_fit_t *fit_out,
                                  int16_t *queries_out, int32_t *status_out, void *stream) {
    const char *who = "s5gpu_path_fit_dev";
    int rc;
    if ((rc = check_shape(who, qpitch, R, wmax, ref)) || (rc = check_refine_params(who, params))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !lo || !hi || !status_in || !fit_out || !status_out) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (mis(queries, 2) || mis(qlen, 4) || mis(ref, 2) || mis(lo, 4) || mis(hi, 4) || mis(status_in, 4) || mis(fit_out, 16) || mis(queries_out, 2) ||
        mis(status_out, 4)) {
        s5gpu_set_error("%s: misaligned argument (fit_out: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    refk::FitArgs A;
    A.queries = queries; A.qpitch = qpitch; A.qlen = qlen; A.ref = ref; A.R = R; A.lo = lo; A.hi = hi; A.status_in = status_in; A.wmax = wmax;
    A.P = *params; A.fit = fit_out; A.queries_out = queries_out; A.status_out = status_out;
    return refk::launch_fit(n, A, (hipStream_t)stream);
}

extern "C" int s5gpu_sdtw_window_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                                     const s5gpu_map_row_t *rows_in, uint32_t pad, uint32_t wmax, void *scratch, size_t scratch_bytes,
                                     s5gpu_map_row_t *rows_out, int32_t *lo, int32_t *hi, int32_t *status, void *stream) {
    const char *who = "s5gpu_sdtw_window_dev";
    int rc;
    if ((rc = check_shape(who, qpitch, R, wmax, ref))) return rc;
    if (pad > refk::PAD_MAX) { s5gpu_set_error("%s: a pad of %u columns (0 .. %u)", who, pad, refk::PAD_MAX); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !rows_in || !scratch || !rows_out || !lo || !hi || !status) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (mis(queries, 2) || mis(qlen, 4) || mis(ref, 2) || mis(rows_in, 16) || mis(scratch, 16) || mis(rows_out, 16) || mis(lo, 4) || mis(hi, 4) || mis(status, 4)) {
        s5gpu_set_error("%s: misaligned argument (rows, scratch: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    if (rows_in == rows_out) { s5gpu_set_error("%s: rows_out is rows_in", who); return S5GPU_ERR_ARG; }
    refk::WinArgs A;
    A.queries = queries; A.qpitch = qpitch; A.qlen = qlen; A.ref = ref; A.R = R; A.rows_in = reinterpret_cast<const dtwk::U4 *>(rows_in); A.gate = nullptr;
    A.pad = pad; A.wmax = wmax; A.scratch = nullptr; A.slot_words = 0; A.rows_out = reinterpret_cast<dtwk::U4 *>(rows_out); A.lo = lo; A.hi = hi;
    A.status = status;
    return window_groups(who, n, A, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" size_t s5gpu_refine_work_bytes(uint32_t n, uint32_t qpitch) {
    if (qpitch == 0 || qpitch > dtwk::QMAX) return 0;
    return work_layout(n, qpitch).bytes;
}

extern "C" int s5gpu_refine_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                                const s5gpu_map_row_t *rows_in, const int32_t *lo_in, const int32_t *hi_in, const int32_t *status_in, uint32_t wmax,
                                const s5gpu_refine_params_t *params, void *scratch, size_t scratch_bytes, void *work, size_t work_bytes, int16_t *queries_out,
                                s5gpu_map_row_t *rows_out, int32_t *lo_out, int32_t *hi_out, s5gpu_fit_t *fit_out, int32_t *status_out, uint32_t *rounds_out,
                                void *stream) {
    const char *who = "s5gpu_refine_dev";
    int rc;
    if ((rc = check_shape(who, qpitch, R, wmax, ref)) || (rc = check_refine_params(who, params))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!queries || !qlen || !rows_in || !lo_in || !hi_in || !status_in || !scratch || !work || !queries_out || !rows_out || !lo_out || !hi_out || !fit_out ||
        !status_out || !rounds_out) {
        s5gpu_set_error("%s: NULL argument", who);
        return S5GPU_ERR_ARG;
    }
    if (mis(queries, 2) || mis(qlen, 4) || mis(ref, 2) || mis(rows_in, 16) || mis(lo_in, 4) || mis(hi_in, 4) || mis(status_in, 4) || mis(scratch, 16) ||
        mis(work, 16) || mis(queries_out, 2) || mis(rows_out, 16) || mis(lo_out, 4) || mis(hi_out, 4) || mis(fit_out, 16) || mis(status_out, 4) ||
        mis(rounds_out, 4)) {
        s5gpu_set_error("%s: misaligned argument (rows, fit_out, scratch, work: 16 bytes)", who);
        return S5GPU_ERR_ARG;
    }
    if ((const void *)queries == (const void *)queries_out || (const void *)rows_in == (const void *)rows_out || lo_in == lo_out || hi_in == hi_out ||
        status_in == status_out) {
        s5gpu_set_error("%s: an output is an input", who);
        return S5GPU_ERR_ARG;
    }
    const Work W = work_layout(n, qpitch);
    if (work_bytes < W.bytes) { s5gpu_set_error("%s: a work area of %zu bytes, %zu are needed", who, work_bytes, W.bytes); return S5GPU_ERR_NOMEM; }
    if (scratch_bytes < s5gpu_sdtw_path_slot_bytes(qpitch, wmax)) {
        s5gpu_set_error("%s: a scratch of %zu bytes, a read needs %zu", who, scratch_bytes, s5gpu_sdtw_path_slot_bytes(qpitch, wmax));
        return S5GPU_ERR_NOMEM;
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t *w = (uint8_t *)work;
    dtwk::U4 *t_rows = (dtwk::U4 *)(w + W.o_rows);
    s5gpu_fit_t *t_fit = (s5gpu_fit_t *)(w + W.o_fit);
    int32_t *t_sf = (int32_t *)(w + W.o_sf), *t_sw = (int32_t *)(w + W.o_sw), *t_lo = (int32_t *)(w + W.o_lo), *t_hi = (int32_t *)(w + W.o_hi);
    int16_t *t_q = (int16_t *)(w + W.o_q);
    refk::RoundArgs B;
    B.qpitch = qpitch; B.qlen = qlen; B.q_in = queries; B.rows_in = reinterpret_cast<const dtwk::U4 *>(rows_in); B.lo_in = lo_in; B.hi_in = hi_in;
    B.status_in = status_in; B.t_q = t_q; B.t_rows = t_rows; B.t_lo = t_lo; B.t_hi = t_hi; B.t_fit = t_fit; B.t_st_fit = t_sf; B.t_st_win = t_sw;
    B.q = queries_out; B.rows = reinterpret_cast<dtwk::U4 *>(rows_out); B.lo = lo_out; B.hi = hi_out; B.fit = fit_out; B.status = status_out;
    B.rounds = rounds_out;
    if ((rc = refk::launch_round(n, B, 0, st))) return rc;
    for (uint32_t round = 1; round <= params->iters; round++) {
        // the fit of the query that came in along the path the read has now, into the trial; a read that has a status keeps it there
        refk::FitArgs F;
        F.queries = queries; F.qpitch = qpitch; F.qlen = qlen; F.ref = ref; F.R = R; F.lo = lo_out; F.hi = hi_out; F.status_in = status_out; F.wmax = wmax;
        F.P = *params; F.fit = t_fit; F.queries_out = t_q; F.status_out = t_sf;
        if ((rc = refk::launch_fit(n, F, st))) return rc;
        // the trial's query in the window around the row the read has now
        refk::WinArgs A;
        A.queries = t_q; A.qpitch = qpitch; A.qlen = qlen; A.ref = ref; A.R = R; A.rows_in = B.rows; A.gate = t_sf; A.pad = params->pad; A.wmax = wmax;
        A.scratch = nullptr; A.slot_words = 0; A.rows_out = t_rows; A.lo = t_lo; A.hi = t_hi; A.status = t_sw;
        if ((rc = window_groups(who, n, A, scratch, scratch_bytes, st))) return rc;
        if ((rc = refk::launch_round(n, B, round, st))) return rc;
    }
    return S5GPU_OK;
}

extern "C" int s5gpu_refine_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
                                  const s5gpu_map_params_t *mp, uint32_t wmax, const s5gpu_refine_params_t *rp, const int16_t *ref_host, uint32_t R,
                                  s5gpu_map_row_t *rows_out, s5gpu_map_row_t *rows_refined_out, s5gpu_fit_t *fit_out, int32_t *lo_out, int32_t *hi_out,
                                  s5gpu_event_t *events_out, int32_t *status_out, uint32_t *rounds_out) {
    const char *who = "s5gpu_refine_batch";
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R,
                                    rows_out && rows_refined_out && fit_out && lo_out && hi_out)))
        return rc;
    if ((rc = dtwk::check_wmax(who, wmax)) || (rc = check_refine_params(who, rp))) return rc;
    if (n == 0) return S5GPU_OK;
    if ((rc = dtwk::path_scratch_check(who, mp->qmax, wmax))) return rc;
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, ep, mp, ref_host, R, F))) return rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m, qmax = mp->qmax;
    const size_t row_i = (size_t)qmax;
    for (uint32_t i = 0; i < n; i++) { rows_refined_out[i] = dtwk::EMPTY_ROW; fit_out[i] = refk::fit_none(); }   // what a record that was dropped keeps
    for (size_t x = 0; x < (size_t)n * row_i; x++) { lo_out[x] = -1; hi_out[x] = -1; }
    if (events_out) memset(events_out, 0, sizeof(s5gpu_event_t) * (size_t)n * row_i);
    if (rounds_out) memset(rounds_out, 0, sizeof(uint32_t) * n);
    // in c->d_gather: what the path tail leaves (rows, path statuses, lo, hi, events), then the refined rows, statuses, rounds, fits, lo and
    // hi, which come back with it in one copy, then the refined queries and the work area, which do not
    dtwk::PathTail T = dtwk::path_layout(m, qmax, true);
    const size_t o_rrow = up(T.bytes, 64), o_rst = o_rrow + up(16ull * m, 16), o_rnd = o_rst + up(4ull * m, 16), o_fit = o_rnd + up(4ull * m, 16);
    const size_t o_rlo = o_fit + 64ull * m, o_rhi = o_rlo + up(4ull * m * qmax, 16), back = o_rhi + up(4ull * m * qmax, 16);
    const size_t o_rq = back, o_work = o_rq + up(2ull * m * qmax, 16);
    T.bytes = o_work + s5gpu_refine_work_bytes(m, qmax);
    if (m) {
        if ((rc = dtwk::path_tail(F, mp, wmax, R, true, T, back))) return rc;
        uint8_t *dg = (uint8_t *)c->d_gather.p;
        const size_t slot = s5gpu_sdtw_path_slot_bytes(qmax, wmax);
        const size_t scratch = slot * m < dtwk::SCRATCH_MAX ? slot * m : dtwk::SCRATCH_MAX / slot * slot;      // (what path_tail reserved in c->d_scan)
        if ((rc = s5gpu_refine_dev(m, F.d_q, qmax, F.d_ql, F.d_ref, R, (const s5gpu_map_row_t *)dg, (const int32_t *)(dg + T.o_lo), (const int32_t *)(dg + T.o_hi),
                                   (const int32_t *)(dg + T.o_pst), wmax, rp, c->d_scan.p, scratch, dg + o_work, T.bytes - o_work, (int16_t *)(dg + o_rq),
                                   (s5gpu_map_row_t *)(dg + o_rrow), (int32_t *)(dg + o_rlo), (int32_t *)(dg + o_rhi), (s5gpu_fit_t *)(dg + o_fit),
                                   (int32_t *)(dg + o_rst), (uint32_t *)(dg + o_rnd), c->st)))
            return rc;
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, back, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
    }
    const uint8_t *h = (const uint8_t *)c->h_out.p;
    dtwk::scatter_rows(F, n, (const s5gpu_map_row_t *)h, (const int32_t *)(h + o_rst), rows_out);
    for (uint32_t k = 0; k < m; k++) {
        const size_t i = F.cur[k];
        rows_refined_out[i] = ((const s5gpu_map_row_t *)(h + o_rrow))[k];
        fit_out[i] = ((const s5gpu_fit_t *)(h + o_fit))[k];
        if (rounds_out) rounds_out[i] = ((const uint32_t *)(h + o_rnd))[k];
        memcpy(lo_out + i * row_i, h + o_rlo + 4 * k * row_i, 4 * row_i);
        memcpy(hi_out + i * row_i, h + o_rhi + 4 * k * row_i, 4 * row_i);
        if (events_out) memcpy(events_out + i * row_i, h + T.o_ev + 16 * k * row_i, 16 * row_i);
    }
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its outputs are empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
