// band_api.hip — host side of the extend calls (include/slow5gpu.h, "extend"; docs/codecs.md §4.21): argument checks and launches of
// s5gpu_event_queries_long_dev and s5gpu_sdtw_band_dev, the size of the latter's scratch, and s5gpu_extend_batch: the front of
// s5gpu_map_batch (dtw_host.h) -> sDTW of the prefix with the start -> the long queries of the event rows that are resident already ->
// the banded alignment from `start`, in groups of consecutive reads whose scratch fits -> one download.
#include <vector>

#include "refine_host.h"

int bandk::check_band_params(const char *who, const s5gpu_band_params_t *p) {
    if (!p) { s5gpu_set_error("%s: NULL band parameters", who); return S5GPU_ERR_ARG; }
    if (!bandk::params_ok(*p)) {
        s5gpu_set_error("%s: band parameters emin %u emax %u (1 <= emin <= emax <= %u) tile_rows %u (64, 128, 256, 512, 1024) band %u (a multiple of 64 in "
                        "64 .. 4096) clip %d (1 .. 32767) scale %g (finite, > 0)", who, p->emin, p->emax, bandk::EMAX, p->tile_rows, p->band, p->clip, p->scale);
        return S5GPU_ERR_ARG;
    }
    return S5GPU_OK;
}

int bandk::check_band_agrees(const char *who, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp) {
    if (bp->skip != mp->skip || bp->scale != mp->scale || bp->clip != mp->clip) {
        s5gpu_set_error("%s: skip, scale and clip of the band parameters are not those of the map parameters (the anchor is a column of the same query)", who);
        return S5GPU_ERR_ARG;
    }
    return S5GPU_OK;
}

using bandk::check_band_params;

namespace {

bool mis(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; }

}  // namespace

extern "C" int s5gpu_event_queries_long_dev(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const int32_t *ev_status,
                                            const s5gpu_band_params_t *p, uint64_t total_rows, int16_t *queries, uint32_t *qlen, int32_t *status,
                                            void *stream) {
    const char *who = "s5gpu_event_queries_long_dev";
    int rc;
    if ((rc = check_band_params(who, p))) return rc;
    if (n == 0) return S5GPU_OK;
    if (!first || !qlen || !status || (total_rows && (!rows || !queries))) { s5gpu_set_error("%s: NULL argument", who); return S5GPU_ERR_ARG; }
    if (mis(rows, 16) || mis(first, 8) || mis(ev_status, 4) || mis(queries, 2) || mis(qlen, 4) || mis(status, 4)) {
        s5gpu_set_error("%s: misaligned argument (rows: 16 bytes, first: 8)", who);
        return S5GPU_ERR_ARG;
    }
    bandk::LongQueryArgs A;
    A.rows = rows; A.first = first; A.ev_status = ev_status; A.total_rows = total_rows; A.skip = p->skip; A.emin = p->emin; A.emax = p->emax;
    A.scale = p->scale; A.clip = p->clip; A.queries = queries; A.qlen = qlen; A.status = status;
    return bandk::launch_queries_long(n, A, (hipStream_t)stream);
}

extern "C" size_t s5gpu_sdtw_band_scratch_bytes(uint32_t n, uint64_t total_rows, uint32_t tile_rows, uint32_t band) {
    if (!bandk::tile_ok(tile_rows) || !bandk::band_ok(band)) return 0;
    return (size_t)bandk::scratch_bytes(bandk::slot_count(total_rows, tile_rows, n), dtwk::path_slot_words(tile_rows, band));
}

extern "C" int s5gpu_sdtw_band_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, const int16_t *ref,
                                   uint32_t R, const int32_t *anchor, const int32_t *status_in, const s5gpu_band_params_t *p, void *scratch,
                                   size_t scratch_bytes, s5gpu_ext_row_t *rows_out, int32_t *lo, int32_t *hi, void *stream) {
    const char *who = "s5gpu_sdtw_band_dev";
    int rc;
    if ((rc = check_band_params(who, p)) || (rc = dtwk::check_ref(who, R))) return rc;
    if (!ref) { s5gpu_set_error("%s: NULL reference", who); return S5GPU_ERR_ARG; }
    if (total_rows > ((uint64_t)1 << 40)) { s5gpu_set_error("%s: %llu rows in all (at most 2^40)", who, (unsigned long long)total_rows); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!first || !qlen || !anchor || !status_in || !scratch || !rows_out || (total_rows && (!queries || !lo || !hi))) {
        s5gpu_set_error("%s: NULL argument", who);
        return S5GPU_ERR_ARG;
    }
    if (mis(queries, 2) || mis(first, 8) || mis(qlen, 4) || mis(ref, 2) || mis(anchor, 4) || mis(status_in, 4) || mis(scratch, 16) || mis(rows_out, 16) ||
        mis(lo, 4) || mis(hi, 4)) {
        s5gpu_set_error("%s: misaligned argument (rows_out, scratch: 16 bytes; first: 8)", who);
        return S5GPU_ERR_ARG;
    }
    const uint64_t slots = bandk::slot_count(total_rows, p->tile_rows, n);
    const uint32_t slot_words = dtwk::path_slot_words(p->tile_rows, p->band);
    const uint64_t need = bandk::scratch_bytes(slots, slot_words);
    if ((uint64_t)scratch_bytes < need) {
        s5gpu_set_error("%s: a scratch of %zu bytes, %llu are needed (%llu slots)", who, scratch_bytes, (unsigned long long)need, (unsigned long long)slots);
        return S5GPU_ERR_NOMEM;
    }
    bandk::BandArgs A;
    A.queries = queries; A.first = first; A.qlen = qlen; A.total_rows = total_rows; A.ref = ref; A.R = R; A.anchor = anchor; A.anchor_stride = 1;
    A.status_in = status_in; A.row0 = 0;
    A.T = p->tile_rows; A.band = p->band; A.scratch = (uint32_t *)scratch; A.slots = slots; A.slot_words = slot_words;
    A.tile_a = (int32_t *)((uint8_t *)scratch + slots * ((uint64_t)slot_words * 256u));
    A.rows_out = rows_out; A.lo = lo; A.hi = hi;
    return bandk::launch_band(n, A, (hipStream_t)stream);
}

// The device side of s5gpu_extend_batch behind a front with m >= 1 reads (band_host.h), queued on the front's stream
int bandk::extend_tail(const char *who, dtwk::MapFront &F, const s5gpu_map_params_t *mp, const s5gpu_band_params_t *bp, size_t scratch_max, uint32_t R,
                       bool events, bool paths_back, size_t rows_cap, size_t scan_min, uint64_t *room_out, ExtTail &E, const s5gpu_refine_params_t *rp) {
    int rc;
    Ctx *c = F.hold.c;
    const uint32_t m = F.m, T = bp->tile_rows;
    const uint64_t total = F.total;
    const uint32_t slot_words = dtwk::path_slot_words(T, bp->band);
    if (scratch_max == 0) scratch_max = (size_t)1 << 30;
    E.first.assign(m + 1u, 0);
    E.too_big.assign(m, 0);
    std::vector<uint64_t> &first = E.first;
    E.o_map = up(32ull * m, 16); E.o_lo = E.o_map + up(16ull * m, 16); E.o_hi = E.o_lo + up(4ull * total, 16); E.o_ev = E.o_hi + up(4ull * total, 16);
    E.back = E.o_ev + (events ? 16ull * total : 0); E.o_q = up(E.back, 16); E.o_ql = E.o_q + up(2ull * total, 16); E.o_st = E.o_ql + up(4ull * m, 16);
    // the host has to know the reads' rows: the room the caller needs, and the groups
    HIP_TRY(hipMemcpyAsync(first.data(), F.d_first, 8ull * (m + 1u), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    uint64_t room = 0;
    for (uint32_t k = 0; k < m; k++) room += bandk::long_qlen(first[k + 1] - first[k], bp->skip, bp->emin, bp->emax);
    if (room > rows_cap) {
        *room_out = room;
        s5gpu_set_error("%s: room for %zu rows, %llu may be needed", who, rows_cap, (unsigned long long)room);
        return S5GPU_ERR_NOMEM;
    }
    size_t gather = E.o_st + 4ull * m, host = paths_back ? E.back : E.o_lo + 4ull * m;
    if (rp) {
        E.r_base = E.r_rows = up(gather, 64); E.r_fit = E.r_rows + 32ull * m; E.r_rnd = E.r_fit + 64ull * m; E.r_lo = E.r_rnd + up(4ull * m, 16);
        E.r_hi = E.r_lo + up(4ull * total, 16); E.r_q = E.r_hi + up(4ull * total, 16); E.r_back = E.r_q + up(2ull * total, 16); E.r_work = E.r_back;
        gather = E.r_work + (size_t)refk::refine_long_work(m, total).bytes;
        host = paths_back ? E.r_back : host + 32ull * m + 16;
    }
    if ((rc = c->d_gather.reserve(gather + 64)) || (rc = c->h_out.reserve(host + 64))) return rc;
    uint8_t *dg = (uint8_t *)c->d_gather.p;
    s5gpu_ext_row_t *d_rows = (s5gpu_ext_row_t *)dg;
    s5gpu_map_row_t *d_map = (s5gpu_map_row_t *)(dg + E.o_map);
    int32_t *d_lo = (int32_t *)(dg + E.o_lo), *d_hi = (int32_t *)(dg + E.o_hi), *d_st = (int32_t *)(dg + E.o_st);
    int16_t *d_q = (int16_t *)(dg + E.o_q);
    uint32_t *d_ql = (uint32_t *)(dg + E.o_ql);
    if ((rc = dtwk::launch_sdtw(m, F.d_q, mp->qmax, F.d_ql, F.d_ref, R, true, d_map, c->st)) ||
        (rc = s5gpu_event_queries_long_dev(m, F.d_rows, F.d_first, F.d_est, bp, total, d_q, d_ql, d_st, c->st)))
        return rc;
    // consecutive reads while their scratch fits; a read that does not fit alone is passed over
    size_t most = scan_min;
    std::vector<uint32_t> cut(1, 0);
    for (uint32_t b = 0; b < m;) {
        uint32_t e = b;
        size_t need = 0;
        while (e < m) {
            const size_t nx = (size_t)bandk::scratch_bytes(bandk::slot_count(first[e + 1] - first[b], T, e + 1u - b), slot_words);
            if (nx > scratch_max) break;
            need = nx;
            e++;
        }
        if (e == b) { E.too_big[b] = 1; e = b + 1; }
        most = need > most ? need : most;
        cut.push_back(e);
        b = e;
    }
    if ((rc = c->d_scan.reserve(most + 64))) return rc;
    if (rp && (rc = refk::long_rounds_fill((int16_t *)(dg + E.r_q), (int32_t *)(dg + E.r_lo), (int32_t *)(dg + E.r_hi), total, c->st))) return rc;
    for (size_t g = 0; g + 1 < cut.size(); g++) {
        const uint32_t b = cut[g], e = cut[g + 1];
        if (E.too_big[b]) continue;
        bandk::BandArgs A;
        A.queries = d_q; A.first = F.d_first + b; A.qlen = d_ql + b; A.total_rows = total; A.ref = F.d_ref; A.R = R;
        A.anchor = &d_map[b].start; A.anchor_stride = sizeof(s5gpu_map_row_t) / sizeof(int32_t); A.status_in = d_st + b; A.row0 = first[b];
        A.T = T; A.band = bp->band; A.scratch = (uint32_t *)c->d_scan.p; A.slots = bandk::slot_count(first[e] - first[b], T, e - b);
        A.slot_words = slot_words; A.tile_a = (int32_t *)((uint8_t *)c->d_scan.p + A.slots * ((uint64_t)slot_words * 256u));
        A.rows_out = d_rows + b; A.lo = d_lo; A.hi = d_hi;
        if ((rc = bandk::launch_band(e - b, A, c->st))) return rc;         // (the stream orders the groups: the scratch is used again)
        if (!rp) continue;
        refk::LongRounds X;
        X.n = e - b; X.queries = d_q; X.first = A.first; X.qlen = A.qlen; X.total_rows = total; X.ref = F.d_ref; X.R = R; X.rows_in = d_rows + b; X.lo_in = d_lo;
        X.hi_in = d_hi; X.row0 = first[b]; X.T = T; X.band = bp->band; X.P = *rp; X.scratch = c->d_scan.p; X.slots = A.slots; X.slot_words = slot_words;
        X.work = dg + E.r_work; X.queries_out = (int16_t *)(dg + E.r_q); X.rows_out = (s5gpu_ext_row_t *)(dg + E.r_rows) + b; X.lo_out = (int32_t *)(dg + E.r_lo);
        X.hi_out = (int32_t *)(dg + E.r_hi); X.fit_out = (s5gpu_fit_t *)(dg + E.r_fit) + b; X.rounds_out = (uint32_t *)(dg + E.r_rnd) + b;
        if ((rc = refk::long_rounds(X, c->st))) return rc;
    }
    return S5GPU_OK;
}

void bandk::scatter_ext_rows(dtwk::MapFront &F, uint32_t n, const ExtTail &E, const uint8_t *h, s5gpu_ext_row_t *rows_out) {
    for (uint32_t i = 0; i < n; i++) rows_out[i] = bandk::row_none(F.status[i]);
    for (uint32_t k = 0; k < F.m; k++) {
        const uint32_t i = F.cur[k];
        rows_out[i] = E.too_big[k] ? bandk::row_none(S5GPU_STATUS_PATH_WIDE) : ((const s5gpu_ext_row_t *)h)[k];
        if (rows_out[i].status != 0) F.status[i] = rows_out[i].status;
    }
}

extern "C" int s5gpu_extend_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_event_params_t *ep,
                                  const s5gpu_map_params_t *mp_in, const s5gpu_band_params_t *bp, size_t scratch_max, const int16_t *ref_host, uint32_t R,
                                  s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *rows_out, uint64_t *ev_first_out, int32_t *lo_out, int32_t *hi_out,
                                  s5gpu_event_t *events_out, size_t rows_cap, int32_t *status_out) {
    const char *who = "s5gpu_extend_batch";
    int rc;
    if ((rc = dtwk::map_front_check(who, n, rec, rec_len, rec_method, sig_method, ep, mp_in, ref_host, R, map_rows_out && rows_out)) ||
        (rc = check_band_params(who, bp)))
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
    // in c->d_gather: the rows, the prefix rows, lo, hi and (wanted) a copy of the event rows, which come back in one copy; behind them the
    // long queries, their lengths and statuses, which do not
    bandk::ExtTail E;
    const uint8_t *h = nullptr;
    if (m) {
        if ((rc = bandk::extend_tail(who, F, &mp, bp, scratch_max, R, events_out != nullptr, true, rows_cap, 0, &ev_first_out[0], E))) return rc;
        uint8_t *dg = (uint8_t *)c->d_gather.p;
        if (events_out && total) HIP_TRY(hipMemcpyAsync(dg + E.o_ev, F.d_rows, 16ull * total, hipMemcpyDeviceToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->h_out.p, dg, E.back, hipMemcpyDeviceToHost, c->st));
        HIP_TRY(hipStreamSynchronize(c->st));
        h = (const uint8_t *)c->h_out.p;
    }
    const std::vector<uint64_t> &first = E.first;
    const size_t o_map = E.o_map, o_lo = E.o_lo, o_hi = E.o_hi, o_ev = E.o_ev;
    dtwk::scatter_rows(F, n, h ? (const s5gpu_map_row_t *)(h + o_map) : nullptr, nullptr, map_rows_out);
    bandk::scatter_ext_rows(F, n, E, h, rows_out);
    uint64_t at = 0;                                                       // the rows of record i: [ev_first_out[i], ev_first_out[i + 1]), in record order
    std::vector<uint32_t> of(n, 0xFFFFFFFFu);
    for (uint32_t k = 0; k < m; k++) of[F.cur[k]] = k;
    for (uint32_t i = 0; i < n; i++) {
        ev_first_out[i] = at;
        const uint32_t Q = rows_out[i].qlen, k = of[i];
        if (Q == 0 || k == 0xFFFFFFFFu) continue;
        memcpy(lo_out + at, h + o_lo + 4 * first[k], 4ull * Q);
        memcpy(hi_out + at, h + o_hi + 4 * first[k], 4ull * Q);
        if (events_out) memcpy(events_out + at, h + o_ev + 16 * (first[k] + bp->skip), 16ull * Q);
        at += Q;
    }
    ev_first_out[n] = at;
    if (status_out) memcpy(status_out, F.status, sizeof(int32_t) * n);
    if (F.corrupt) { s5gpu_set_error("%s: at least one record is corrupt (its status is not 0 and its outputs are empty)", who); return S5GPU_ERR_DATA; }
    return S5GPU_OK;
}
