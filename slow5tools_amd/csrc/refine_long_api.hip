// refine_long_api.hip — host side of the whole-read refine calls (include/slow5gpu.h, "refine, whole reads"; docs/codecs.md §4.24):
// argument checks and launches of s5gpu_path_fit_long_dev, the rounds of s5gpu_extend_refine_dev (refk::long_rounds, which
// bandk::extend_tail runs behind each group's band call too), and s5gpu_extend_refine_batch: the chain of s5gpu_extend_batch with the
// rounds, and two downloads.
#include <vector>

#include "refine_host.h"

namespace {

bool mis(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

int check_long_shape(const char *who, uint32_t R, const int16_t *ref, uint64_t total_rows) {
    int rc;
    if ((rc = dtwk::check_ref(who, R))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (total_rows > pilek::LONG_ROWS_MAX) { s5gpu_set_error("%s: %llu rows in all (at most 2^40)", who, (unsigned long long)total_rows); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

}  // namespace

extern "C" size_t s5gpu_path_fit_long_work_bytes(uint32_t n, uint64_t total_rows) {
    if (total_rows > pilek::LONG_ROWS_MAX) return 0;
    return (size_t)refk::fit_long_work(n, total_rows).bytes;
}

extern "C" size_t s5gpu_extend_refine_work_bytes(uint32_t n, uint64_t total_rows) {
    if (total_rows > pilek::LONG_ROWS_MAX) return 0;
    return (size_t)refk::refine_long_work(n, total_rows).bytes;
}

extern "C" int s5gpu_path_fit_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, const int16_t *ref,
                                       uint32_t R, const int32_t *lo, const int32_t *hi, const int32_t *status_in, const s5gpu_refine_params_t *params, void *work,
                                       size_t work_bytes, s5gpu_fit_t *fit_out, int16_t *queries_out, int32_t *status_out, void *stream) {
    const char *who = "s5gpu_path_fit_long_dev";
    int rc;
    if ((rc = check_long_shape(who, R, ref, total_rows)) || (rc = refk::check_refine_params(who, params))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!first || !qlen || !status_in || !work || !fit_out || !status_out || (total_rows && (!queries || !lo || !hi))) {
        s5gpu_set_error("%s: NULL argument", who);
        return S5GPU_ERR_ARG;
    }
    if (mis(queries, 2) || mis(first, 8) || mis(qlen, 4) || mis(ref, 2) || mis(lo, 4) || mis(hi, 4) || mis(status_in, 4) || mis(work, 16) || mis(fit_out, 16) ||
        mis(queries_out, 2) || mis(status_out, 4)) {
        s5gpu_set_error("%s: misaligned argument (first: 8 bytes; fit_out, work: 16)", who);
        return S5GPU_ERR_ARG;
    }
    if (queries_out && (const void *)queries_out == (const void *)queries) { s5gpu_set_error("%s: queries_out is queries", who); return S5GPU_ERR_ARG; }
    if (status_out == status_in) { s5gpu_set_error("%s: status_out is status_in", who); return S5GPU_ERR_ARG; }
    const uint64_t need = refk::fit_long_work(n, total_rows).bytes;
    if ((uint64_t)work_bytes < need) {
        s5gpu_set_error("%s: a work area of %zu bytes, %llu are needed", who, work_bytes, (unsigned long long)need);
        return S5GPU_ERR_NOMEM;
    }
    hipStream_t st = (hipStream_t)stream;
    if (queries_out && total_rows && (refk::long_passes() & 8u)) HIP_TRY(hipMemsetAsync(queries_out, 0, 2ull * total_rows, st));
    refk::FitLongArgs F;
    F.A.n = n; F.A.queries = queries; F.A.first = first; F.A.qlen = qlen; F.A.total_rows = total_rows; F.A.ref = ref; F.A.R = R; F.A.lo = lo; F.A.hi = hi;
    F.A.status = status_in; F.A.events = nullptr; F.A.ev_skip = 0; F.A.work = work; F.A.acc = nullptr;
    F.P = *params; F.fit = fit_out; F.queries_out = queries_out; F.status_out = status_out;
    return refk::launch_fit_long(F, st);
}

int refk::long_rounds_fill(int16_t *queries_out, int32_t *lo_out, int32_t *hi_out, uint64_t total_rows, hipStream_t st) {
    if (total_rows == 0 || !(refk::long_passes() & 16u)) return S5GPU_OK;
    HIP_TRY(hipMemsetAsync(queries_out, 0, 2ull * total_rows, st));
    HIP_TRY(hipMemsetAsync(lo_out, 0xFF, 4ull * total_rows, st));         // (every byte 0xFF: -1)
    HIP_TRY(hipMemsetAsync(hi_out, 0xFF, 4ull * total_rows, st));
    return S5GPU_OK;
}

int refk::long_rounds(const LongRounds &X, hipStream_t st) {
    if (X.n == 0) return S5GPU_OK;
    int rc;
    const RefineLongWork W = refine_long_work(X.n, X.total_rows);
    uint8_t *w = (uint8_t *)X.work;
    s5gpu_ext_row_t *t_rows = (s5gpu_ext_row_t *)(w + W.o_rows);
    s5gpu_fit_t *t_fit = (s5gpu_fit_t *)(w + W.o_fit);
    int32_t *t_sf = (int32_t *)(w + W.o_sf), *cur[2] = {(int32_t *)(w + W.o_st0), (int32_t *)(w + W.o_st1)};
    int32_t *t_lo = (int32_t *)(w + W.o_lo), *t_hi = (int32_t *)(w + W.o_hi);
    int16_t *t_q = (int16_t *)(w + W.o_q);
    // round 0: the statuses that came in -> cur[1]; the verdicts of the paths that came in; the copies, and the statuses -> cur[0]
    RoundLongArgs B;
    B.A.n = X.n; B.A.queries = X.queries; B.A.first = X.first; B.A.qlen = X.qlen; B.A.total_rows = X.total_rows; B.A.ref = X.ref; B.A.R = X.R;
    B.A.lo = X.lo_in; B.A.hi = X.hi_in; B.A.status = cur[1]; B.A.events = nullptr; B.A.ev_skip = 0; B.A.work = X.work; B.A.acc = nullptr;
    B.rows_in = X.rows_in; B.t_q = t_q; B.t_rows = t_rows; B.t_lo = t_lo; B.t_hi = t_hi; B.t_fit = t_fit; B.t_sf = t_sf;
    B.q = X.queries_out; B.rows = X.rows_out; B.lo = X.lo_out; B.hi = X.hi_out; B.fit = X.fit_out; B.rounds = X.rounds_out;
    B.cur_in = cur[1]; B.cur_out = cur[0];
    if ((rc = launch_gate_long(X.n, X.rows_in, cur[1], st)) || (rc = launch_long_verdicts(B.A, st)) || (rc = launch_round_long(B, 0, st))) return rc;
    for (uint32_t round = 1; round <= X.P.iters; round++) {
        const int32_t *has = cur[(round - 1u) & 1u];
        // the fit of the query that came in along the path the read has now, and q' from it, into the trial; a read that has a status
        // keeps it there
        FitLongArgs F;
        F.A = B.A; F.A.lo = X.lo_out; F.A.hi = X.hi_out; F.A.status = has;
        F.P = X.P; F.fit = t_fit; F.queries_out = t_q; F.status_out = t_sf;
        if ((rc = launch_fit_long(F, st))) return rc;
        // the trial's query in the band from `start` of the row the read has now; the fit's status is the gate
        bandk::BandArgs A;
        A.queries = t_q; A.first = X.first; A.qlen = X.qlen; A.total_rows = X.total_rows; A.ref = X.ref; A.R = X.R;
        A.anchor = &X.rows_out[0].start; A.anchor_stride = sizeof(s5gpu_ext_row_t) / sizeof(int32_t); A.status_in = t_sf; A.row0 = X.row0;
        A.T = X.T; A.band = X.band; A.scratch = (uint32_t *)X.scratch; A.slots = X.slots; A.slot_words = X.slot_words;
        A.tile_a = (int32_t *)((uint8_t *)X.scratch + X.slots * ((uint64_t)X.slot_words * 256u));
        A.rows_out = t_rows; A.lo = t_lo; A.hi = t_hi;
        if ((long_passes() & 32u) && (rc = bandk::launch_band(X.n, A, st))) return rc;
        B.A.status = has; B.cur_in = has; B.cur_out = cur[round & 1u];
        if ((rc = launch_round_long(B, round, st))) return rc;
    }
    return S5GPU_OK;
}

extern "C" int s5gpu_extend_refine_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, const int16_t *ref,
                                       uint32_t R, const s5gpu_ext_row_t *rows_in, const int32_t *lo_in, const int32_t *hi_in, const s5gpu_band_params_t *bp,
                                       const s5gpu_refine_params_t *rp, void *scratch, size_t scratch_bytes, void *work, size_t work_bytes, int16_t *queries_out,
                                       s5gpu_ext_row_t *rows_out, int32_t *lo_out, int32_t *hi_out, s5gpu_fit_t *fit_out, uint32_t *rounds_out, void *stream) {
    const char *who = "s5gpu_extend_refine_dev";
    int rc;
    if ((rc = bandk::check_band_params(who, bp)) || (rc = refk::check_refine_params(who, rp)) || (rc = check_long_shape(who, R, ref, total_rows))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!first || !qlen || !rows_in || !scratch || !work || !rows_out || !fit_out || !rounds_out ||
        (total_rows && (!queries || !lo_in || !hi_in || !queries_out || !lo_out || !hi_out))) {
        s5gpu_set_error("%s: NULL argument", who);
        return S5GPU_ERR_ARG;
    }
    if (mis(queries, 2) || mis(first, 8) || mis(qlen, 4) || mis(ref, 2) || mis(rows_in, 16) || mis(lo_in, 4) || mis(hi_in, 4) || mis(scratch, 16) || mis(work, 16) ||
        mis(queries_out, 2) || mis(rows_out, 16) || mis(lo_out, 4) || mis(hi_out, 4) || mis(fit_out, 16) || mis(rounds_out, 4)) {
        s5gpu_set_error("%s: misaligned argument (rows, fit_out, scratch, work: 16 bytes; first: 8)", who);
        return S5GPU_ERR_ARG;
    }
    if ((queries_out && (const void *)queries == (const void *)queries_out) || (const void *)rows_in == (const void *)rows_out || (lo_out && lo_in == lo_out) ||
        (hi_out && hi_in == hi_out)) {
        s5gpu_set_error("%s: an output is an input", who);
        return S5GPU_ERR_ARG;
    }
    const uint64_t slots = bandk::slot_count(total_rows, bp->tile_rows, n);
    const uint32_t slot_words = dtwk::path_slot_words(bp->tile_rows, bp->band);
    const uint64_t need = bandk::scratch_bytes(slots, slot_words), wneed = refk::refine_long_work(n, total_rows).bytes;
    if ((uint64_t)scratch_bytes < need) {
        s5gpu_set_error("%s: a scratch of %zu bytes, %llu are needed (%llu slots)", who, scratch_bytes, (unsigned long long)need, (unsigned long long)slots);
        return S5GPU_ERR_NOMEM;
    }
    if ((uint64_t)work_bytes < wneed) {
        s5gpu_set_error("%s: a work area of %zu bytes, %llu are needed", who, work_bytes, (unsigned long long)wneed);
        return S5GPU_ERR_NOMEM;
    }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = refk::long_rounds_fill(queries_out, lo_out, hi_out, total_rows, st))) return rc;
    refk::LongRounds X;
    X.n = n; X.queries = queries; X.first = first; X.qlen = qlen; X.total_rows = total_rows; X.ref = ref; X.R = R; X.rows_in = rows_in; X.lo_in = lo_in;
    X.hi_in = hi_in; X.row0 = 0; X.T = bp->tile_rows; X.band = bp->band; X.P = *rp; X.scratch = scratch; X.slots = slots; X.slot_words = slot_words; X.work = work;
    X.queries_out = queries_out; X.rows_out = rows_out; X.lo_out = lo_out; X.hi_out = hi_out; X.fit_out = fit_out; X.rounds_out = rounds_out;
    return refk::long_rounds(X, st);
}

extern "C" int s5gpu_extend_refine_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
                                         const s5gpu_map_params_t *mp_in, const s5gpu_band_params_t *bp, const s5gpu_refine_params_t *rp, size_t scratch_max,
                                         const int16_t *ref_host, uint32_t R, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *rows_first_out,
                                         s5gpu_ext_row_t *rows_out, uint64_t *ev_first_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out,
                                         int16_t *queries_out, size_t rows_cap, s5gpu_fit_t *fit_out, uint32_t *rounds_out, int32_t *status_out) {
    const char *who = "s5gpu_extend_refine_batch";
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp_in, ref_host, R, map_rows_out && rows_out && rows_first_out && fit_out)) ||
        (rc = bandk::check_band_params(who, bp)) || (rc = refk::check_refine_params(who, rp)))
        return rc;
    if (!ev_first_out || (rows_cap && (!lo_out || !hi_out))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if ((rc = bandk::check_band_agrees(who, mp_in, bp))) return rc;
    if (n == 0) { ev_first_out[0] = 0; return S5GPU_OK; }
    if (s5host::n_devices() == 0) return S5GPU_ERR_NODEV;
    s5gpu_map_params_t mp = *mp_in;
    mp.want_start = 1;                                                     // the anchor is the start
    dtwk::MapFront F;
    if ((rc = dtwk::map_front(n, rec, rec_len, rec_method, sig_method, ep, &mp, ref_host, R, F))) return rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m;
    const uint64_t total = F.total;
    // in c->d_gather: what s5gpu_extend_batch leaves there (the first rows, the prefix rows, the first paths and the event rows come back
    // in one copy), and behind it the refined block, which comes back in a second
    bandk::ExtTail E;
    const uint8_t *h = nullptr, *hr = nullptr;
    if (m) {
        if ((rc = bandk::extend_tail(who, F, &mp, bp, scratch_max, R, events_out != nullptr, true, rows_cap, 0, &ev_first_out[0], E, rp))) return rc;
        uint8_t *dg = (uint8_t *)c->d_gather.p;
        if (events_out && total) HIP_TRY(hipMemcpyAsync(dg + E.o_ev, F.d_rows, 16ull * total, hipMemcpyDeviceToDevice, c->st));
        // (the first paths are not wanted: the rows and the prefix rows, then the event rows)
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, E.o_lo, hipMemcpyDeviceToHost, c->st));
        if (events_out && total) HIP_TRY(hipMemcpyAsync((uint8_t *)c->h_out.p + E.o_ev, dg + E.o_ev, 16ull * total, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipMemcpyAsync((uint8_t *)c->h_out.p + E.r_base, dg + E.r_base, E.r_back - E.r_base, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        h = (const uint8_t *)c->h_out.p;
        hr = h;
    }
    const std::vector<uint64_t> &first = E.first;
    dtwk::scatter_rows(F, n, h ? (const s5gpu_map_row_t *)(h + E.o_map) : nullptr, nullptr, map_rows_out);
    {   // the first rows, without their statuses' way into F.status: a read's status is its refined row's
        std::vector<int32_t> keep(F.status, F.status + n);
        bandk::scatter_ext_rows(F, n, E, h, rows_first_out);
        memcpy(F.status, keep.data(), sizeof(int32_t) * n);
    }
    bandk::scatter_ext_rows(F, n, E, hr ? hr + E.r_rows : nullptr, rows_out);
    for (uint32_t i = 0; i < n; i++) fit_out[i] = refk::fit_none();
    if (rounds_out) memset(rounds_out, 0, sizeof(uint32_t) * n);
    uint64_t at = 0;                                                       // the rows of record i: [ev_first_out[i], ev_first_out[i + 1]), in record order
    std::vector<uint32_t> of(n, 0xFFFFFFFFu);
    for (uint32_t k = 0; k < m; k++) of[F.cur[k]] = k;
    for (uint32_t i = 0; i < n; i++) {
        ev_first_out[i] = at;
        const uint32_t Q = rows_out[i].qlen, k = of[i];
        if (k != 0xFFFFFFFFu && !E.too_big[k]) {
            fit_out[i] = ((const s5gpu_fit_t *)(hr + E.r_fit))[k];
            if (rounds_out) rounds_out[i] = ((const uint32_t *)(hr + E.r_rnd))[k];
        }
        if (Q == 0 || k == 0xFFFFFFFFu) continue;
        memcpy(lo_out + at, hr + E.r_lo + 4 * first[k], 4ull * Q);
        memcpy(hi_out + at, hr + E.r_hi + 4 * first[k], 4ull * Q);
        if (queries_out) memcpy(queries_out + at, hr + E.r_q + 2 * first[k], 2ull * Q);
        if (events_out) memcpy(events_out + at, h + E.o_ev + 16 * (first[k] + bp->skip), 16ull * Q);
        at += Q;
    }
    ev_first_out[n] = at;
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its outputs are empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
