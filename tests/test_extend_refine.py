"""refine over whole reads (docs/codecs.md §4.24; slow5tools_amd/csrc/refine_long_kernels.hip): the restatement's known answers, the headers'
plain C++ (refine_dev.h, and the walk of ragged_dev.h: every segment is resolved by seg_item, as in the kernels) on the CPU (also under ASan and
UBSan) against it, the planted case, refused arguments, exports; and on the device the fit, the rounds, the chain, pileup and contrast, all
bit for bit against extend_refine_ref.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import contrast_ref as cr
import extend_refine_ref as er
import oracle_bind as ob
from chain_common import DEFAULT_GRID, DEFAULT_SEG, DEFAULT_SORT, DNA, EVENT, EXT_ROW, FIT, FIT_FLAT, FIT_RANGE, PATH_ROW, QUERY_SHORT, ROOT
from chain_common import host_build, levels_signal, pile_lines, record, synth_file, to_dev
from chain_common import gpu  # noqa: F401
from dtw_ref import quant_ref
from extend_ref import MIXED_Q, QLENS, RLENS, SHAPES, band_ref, bparams, tracking_read
from extend_refine_ref import fit_long_ref, refine_long_ref
from pileup_ref import LongCase, pileup_long_ref, table_bytes
from refine_ref import FIT_NONE, c_params, params, params_bytes

NEW_CALLS = ["s5gpu_path_fit_long_work_bytes", "s5gpu_path_fit_long_dev", "s5gpu_extend_refine_work_bytes", "s5gpu_extend_refine_dev",
             "s5gpu_extend_refine_batch", "s5gpu_pileup_set_refine", "s5gpu_contrast_set_refine"]
PLANTED_SEEDS = [1, 2, 3, 4, 5, 6, 7, 8]
PLANTED_SHAPES = [(64, 128, 1500, 4096), (256, 512, 3000, 8192)]           # (tile_rows, band, events, levels)
PLANTED_SHARE, PLANTED_COST = 0.995, 0.2                                   # the floors of the issue
PLANTED_TRACKS = 0.873                                                     # the least share "before" of the prototype: below it a read does not "mostly track"


def fit_tuple(f):
    return tuple(f.tolist()) if hasattr(f, "tolist") else tuple(f)


# ---------------------------------------------------------------------------------------------------------------- hand-made cases

def one_read(q, ref, lo, hi, status=0, first=None, qlen=None, row=None):
    """a LongCase of one read and its EXT_ROW"""
    Q = len(q)
    case = LongCase(q, [0, Q] if first is None else first, [Q if qlen is None else qlen], ref, lo, hi, [status])
    rows = np.zeros(1, dtype=EXT_ROW)
    rows[0] = row if row is not None else (er.row_none(status) if status or not Q else (0, Q, 1, int(lo[0]), int(hi[-1]), 0, 0))
    return case, rows


def hand_cases():
    """-> {name: (case, rows, P)}: the hand-made inputs of the issue"""
    out = {}
    ref = np.array([3, -2, 7, 7, 1, 0, 5, 9, -4, 6], dtype=np.int16)
    # a one-row read over three columns: n = 3 < min_cells
    out["one row"] = one_read([4], ref, [2], [4]) + (params(),)
    # den = 0: every row holds the same level
    out["flat"] = one_read([5] * 20, ref, np.arange(20) // 2, np.arange(20) // 2) + (params(min_cells=2),)
    # n = min_cells - 1 and n = min_cells: 15 and 16 cells on a diagonal where r = 2 q + 1 exactly
    for n in (15, 16):
        q = np.arange(-8, -8 + n, dtype=np.int16)
        out["cells %d" % n] = one_read(q, (2 * q + 1).astype(np.int16), np.arange(n), np.arange(n)) + (params(),)
    # slopes just inside and just outside [a_min, a_max]: r = 2 q exactly, a = 2
    q = np.arange(-10, 10, dtype=np.int16)
    rr = (2 * q).astype(np.int16)
    out["slope inside"] = one_read(q, rr, np.arange(20), np.arange(20)) + (params(a_max=2.0),)
    out["slope outside"] = one_read(q, rr, np.arange(20), np.arange(20)) + (params(a_max=np.nextafter(2.0, 0.0)),)
    out["slope below"] = one_read(q, rr, np.arange(20), np.arange(20)) + (params(a_min=np.nextafter(2.0, 3.0), a_max=4.0),)
    # |b| at b_max: r = q + 7 exactly, b = 7
    rb = (q + 7).astype(np.int16)
    out["shift at b_max"] = one_read(q, rb, np.arange(20), np.arange(20)) + (params(b_max=7.0),)
    out["shift above b_max"] = one_read(q, rb, np.arange(20), np.arange(20)) + (params(b_max=np.nextafter(7.0, 0.0)),)
    # one bad row in the last segment of a read of 200 rows (segments of 64: rows 192 .. 199): nothing of it is counted
    rng = np.random.default_rng(5)
    q, r, anchor = tracking_read(rng, 200, 300)
    w = band_ref(q, r, anchor, 64, 128)
    lo, hi = w["lo"].copy(), w["hi"].copy()
    hi[197] = hi[197] + 2                                                   # row 198 no longer begins where row 197 ended
    out["bad row"] = (LongCase(q, [0, 200], [200], r, lo, hi, [0]), np.array([w["row"]], dtype=EXT_ROW), params())
    # Q = 0, an incoming status, and a layout with `first` out of order (its neighbour is fine)
    out["no query"] = one_read([], ref, [], [], first=[0, 3], qlen=0) + (params(),)
    c = LongCase(q, [0, 200], [200], r, w["lo"], w["hi"], [7])
    out["status in"] = (c, np.array([er.row_none(7)], dtype=EXT_ROW), params())
    q2 = np.concatenate([q, q])
    c = LongCase(q2, [200, 0, 400], [200, 200], r, np.concatenate([w["lo"], w["lo"]]), np.concatenate([w["hi"], w["hi"]]), [0, 0])
    out["first out of order"] = (c, np.array([w["row"], w["row"]], dtype=EXT_ROW), params())
    return out


def test_restatement_known_answers():
    """fit_long_ref and refine_long_ref on inputs small enough to do by hand"""
    H = hand_cases()

    def fit_of(name):
        case, rows, P = H[name]
        fit, q1, st = fit_long_ref(case, P)
        return fit, q1, st
    # one row, columns 2 .. 4 (7, 7, 1) against q = 4: the sums by hand; three cells are fewer than min_cells
    fit, q1, st = fit_of("one row")
    assert st.tolist() == [FIT_FLAT] and fit_tuple(fit[0]) == (1.0, 0.0, 3, 12, 15, 48, 60, 99) and not q1.any()
    fit, q1, st = fit_of("flat")
    assert st.tolist() == [FIT_FLAT] and fit[0]["n"] == 20 and fit[0]["n"] * fit[0]["sqq"] == fit[0]["sq"] ** 2
    assert fit_of("cells 15")[2].tolist() == [FIT_FLAT] and fit_of("cells 16")[2].tolist() == [0]
    fit, q1, st = fit_of("slope inside")
    assert st.tolist() == [0] and (fit[0]["a"], fit[0]["b"]) == (2.0, 0.0) and q1.tolist() == (2 * np.arange(-10, 10)).tolist()
    for name in ("slope outside", "slope below", "shift above b_max"):
        fit, q1, st = fit_of(name)
        assert st.tolist() == [FIT_RANGE] and (fit[0]["a"], fit[0]["b"]) == (1.0, 0.0) and fit[0]["n"] == 20 and not q1.any(), name
    fit, q1, st = fit_of("shift at b_max")
    assert st.tolist() == [0] and (fit[0]["a"], fit[0]["b"]) == (1.0, 7.0)
    fit, q1, st = fit_of("bad row")
    assert st.tolist() == [PATH_ROW] and fit_tuple(fit[0]) == FIT_NONE and not q1.any()
    fit, q1, st = fit_of("no query")
    assert st.tolist() == [0] and fit_tuple(fit[0]) == FIT_NONE
    fit, q1, st = fit_of("status in")
    assert st.tolist() == [7] and fit_tuple(fit[0]) == FIT_NONE and not q1.any()
    fit, q1, st = fit_of("first out of order")
    assert st.tolist() == [PATH_ROW, 0] and fit_tuple(fit[0]) == FIT_NONE and fit[1]["n"] >= 200 and not q1[200:].any() and q1[:200].any()
    # the rounds: a read that is not fitted has no result and its status; one whose fit is refused keeps the copies of what came in
    for name, status in (("bad row", PATH_ROW), ("status in", 7), ("no query", 0)):
        case, rows, P = H[name]
        out = refine_long_ref(case, rows, 64, 128, P)
        assert tuple(out["rows"][0].tolist()) == er.row_none(status) and out["rounds"][0] == 0 and fit_tuple(out["fit"][0]) == FIT_NONE, name
        assert not out["q"].any() and (out["lo"] == -1).all() and (out["hi"] == -1).all(), name
    case, rows, P = H["slope outside"]
    out = refine_long_ref(case, rows, 64, 128, P)
    assert out["rows"][0]["status"] == FIT_RANGE and out["rows"][0]["cost"] == rows[0]["cost"] and out["rounds"][0] == 0 and fit_tuple(out["fit"][0]) == FIT_NONE
    assert np.array_equal(out["q"], case.q) and np.array_equal(out["lo"], case.lo) and np.array_equal(out["hi"], case.hi)
    case, rows, P = H["first out of order"]
    out = refine_long_ref(case, rows, 64, 128, P)
    assert out["rows"]["status"].tolist() == [PATH_ROW, 0] and out["rounds"].tolist() == [0, 2] and (out["lo"][200:] == -1).all() and (out["lo"][:200] >= 0).all()
    # r = 2 q exactly: one round makes q' = r, the cost 0, and the second round fits a = 1, b = 0 along it... of the query that came in: a = 2 again
    case, rows, P = H["slope inside"]
    rows[0] = band_ref(case.q, case.ref, 0, 64, 64)["row"]
    t = []
    out = refine_long_ref(case, rows, 64, 64, P, trace=t)
    assert out["rows"][0]["cost"] == 0 and out["rounds"][0] == 2 and (out["fit"][0]["a"], out["fit"][0]["b"]) == (2.0, 0.0) and np.array_equal(out["q"], case.ref)
    assert len(t) == 3 and t[1]["out"]["rounds"][0] == 1 and t[0]["out"]["rounds"][0] == 0 and np.array_equal(t[0]["out"]["q"], case.q)


# ---------------------------------------------------------------------------------------------------------------- the header's code on the CPU

REFINE_LONG_HOST = r'''
// The plain C++ of the whole-read refine in refine_dev.h and ragged_dev.h (§4.24) on the CPU, the way the kernels use it.  A batch of in.bin:
// n, S, iters, shuffle, total, R, the 40 bytes of the refine parameters, first[n + 1], qlen[n], q0[total], ref[R], rows_in[n], lo_in[total],
// hi_in[total], and for every round j = 1 .. iters what the band call left of the trial: t_rows[n], t_lo[total], t_hi[total] (the band
// kernel is not part of this program).  Every array is allocated at exactly its size with a guard word either side, poisoned under ASan.
// Segments are walked in an order shuffled by `shuffle`, 64 lanes each.  out.bin gets, per batch: what s5gpu_path_fit_long_dev gives for
// (lo_in, hi_in, the rows' statuses): fit[n], status[n], q'[total]; then round 0's outputs q, rows, lo, hi, fit, rounds, cur; then per
// round the trial's fit[n], sf[n], q'[total] and the outputs again.
#define S5_PILEUP_HOST
#include "refine_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) __asan_poison_memory_region((p), (n))
#define UNPOISON(p, n) __asan_unpoison_memory_region((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif
using namespace pilek;
using namespace refk;

template <class T>
struct Arr {
    uint64_t *raw; T *p; size_t n, words;
    explicit Arr(size_t count) : n(count) {
        words = (count * sizeof(T) + 7) / 8;
        raw = (uint64_t *)malloc((words + 2) * 8);
        if (!raw) abort();
        memset(raw, 0, (words + 2) * 8);
        raw[0] = 0x5A5A5A5A5A5A5A5Aull; raw[words + 1] = 0x5A5A5A5A5A5A5A5Aull;
        p = (T *)(raw + 1);
        // (the tail of the last word behind count * sizeof(T) is poisoned too: the array ends at exactly its size)
        POISON(raw, 8); POISON((char *)p + count * sizeof(T), (words + 1) * 8 - count * sizeof(T));
    }
    ~Arr() {
        UNPOISON(raw, (words + 2) * 8);
        if (raw[0] != 0x5A5A5A5A5A5A5A5Aull || raw[words + 1] != 0x5A5A5A5A5A5A5A5Aull) abort();
        free(raw);
    }
    void fill(T v) { for (size_t i = 0; i < n; i++) p[i] = v; }
    bool read(FILE *f) { return fread(p, sizeof(T), n, f) == n; }
    void write(FILE *o) const { fwrite(p, sizeof(T), n, o); }
    Arr(const Arr &) = delete;
};

struct Batch {
    uint32_t n, S, R;
    uint64_t total;
    const uint64_t *first; const uint32_t *qlen; const int16_t *q0, *ref;
};
// segment g of P's order through seg_item of ragged_dev.h, the kernels' resolver (no read carried: the order is shuffled), held to
// seg_find, seg_next and the rows' bounds every time
static Seg seg_of(const Batch &B, const uint64_t *P, uint64_t g) {
    const PileLongArgs A = {B.n, B.q0, B.first, B.qlen, B.total};           // (the rest is not the resolver's)
    const LongPtrs L = {nullptr, const_cast<uint64_t *>(P)};
    Seg s = seg_none(B.n);
    if (!seg_item(A, B.S, L, false, g, &s) || s.k != seg_find(P, B.n, g) || s.k != seg_next(P, B.n, 0u, g) || s.r0 >= s.r1 || s.r1 > B.qlen[s.k] || s.r1 - s.r0 > B.S) abort();
    return s;
}

static uint32_t rnd(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// the plan and the check: verdict[n], P[n + 1]; the segments of the check in shuffled order, resolved by seg_item
static void verdicts(const Batch &B, const int32_t *status, const int32_t *lo, const int32_t *hi, uint32_t *verdict, uint64_t *P, std::vector<uint64_t> &order, uint32_t shuffle) {
    uint64_t at = 0;
    for (uint32_t k = 0; k < B.n; k++) {
        verdict[k] = long_verdict(B.first[k], B.first[k + 1], B.qlen[k], status[k], B.total, 0u);
        P[k] = at;
        at += verdict[k] == V_USED ? segs_of(B.qlen[k], B.S) : 0u;
    }
    P[B.n] = at;
    order.resize(at);
    for (uint64_t g = 0; g < at; g++) order[g] = g;
    uint32_t s = shuffle;
    for (uint64_t g = at; g > 1; g--) { const uint64_t j = rnd(s) % g; const uint64_t t = order[g - 1]; order[g - 1] = order[j]; order[j] = t; }
    for (uint64_t x = 0; x < at; x++) {
        const Seg s = seg_of(B, P, order[x]);
        const uint32_t k = s.k, r0 = s.r0, r1 = s.r1;
        const uint64_t f = B.first[k];
        bool ok = true;
        for (uint32_t lane = 0; lane < 64; lane++) ok = seg_rows_ok(r0, r1, lane, 64u, lo + f, hi + f, B.R) && ok;
        if (!ok) verdict[k] |= V_BAD;
    }
}

// launch_fit_long: the sums by segment and lane, the solve, q' for the reads whose status is 0 (out is written nowhere else)
static void fit_long(const Batch &B, const s5gpu_refine_params_t &Pm, const int32_t *status, const int32_t *lo, const int32_t *hi, uint32_t shuffle, uint32_t *verdict,
                     uint64_t *P, std::vector<uint64_t> &order, s5gpu_fit_t *fit, int32_t *st_out, int16_t *out) {
    verdicts(B, status, lo, hi, verdict, P, order, shuffle);
    Arr<Sums> sums(B.n);
    for (uint64_t x = 0; x < order.size(); x++) {
        const Seg s = seg_of(B, P, order[x]);
        const uint32_t k = s.k, r0 = s.r0, r1 = s.r1;
        if (verdict[k] != V_USED) continue;
        const uint64_t f = B.first[k];
        Sums part = {0, 0, 0, 0, 0, 0};
        for (uint32_t lane = 0; lane < 64; lane++) seg_sums(r0, r1, lane, 64u, lo + f, hi + f, B.q0 + f, B.ref, B.R, part);
        sums_add(sums.p[k], part);
    }
    for (uint32_t k = 0; k < B.n; k++) st_out[k] = long_fit_status(verdict[k], status[k], sums.p[k], Pm, &fit[k]);
    for (uint64_t x = 0; x < order.size(); x++) {
        const Seg s = seg_of(B, P, order[x]);
        const uint32_t k = s.k, r0 = s.r0, r1 = s.r1;
        if (verdict[k] != V_USED || st_out[k] != 0) continue;
        const uint64_t f = B.first[k];
        for (uint32_t i = r0; i < r1; i++) out[f + i] = requant_one(B.q0[f + i], fit[k].a, fit[k].b, Pm.clip);
    }
}

static int one_batch(FILE *f, FILE *o) {
    uint32_t h[4];
    if (fread(h, 4, 4, f) != 4) return 1;
    Batch B;
    B.n = h[0]; B.S = h[1];
    const uint32_t iters = h[2], shuffle = h[3];
    s5gpu_refine_params_t Pm;
    if (fread(&B.total, 8, 1, f) != 1 || fread(&B.R, 4, 1, f) != 1 || fread(&Pm, sizeof Pm, 1, f) != 1 || !params_ok(Pm) || B.n < 1 || B.R < 1) return -1;
    const size_t n = B.n, total = (size_t)B.total;
    Arr<uint64_t> first(n + 1), P(n + 1);
    Arr<uint32_t> qlen(n), verdict(n), rounds(n);
    Arr<int16_t> q0(total), ref(B.R), q1(total), t_q(total), q(total);
    Arr<s5gpu_ext_row_t> rows_in(n), t_rows(n), rows(n);
    Arr<int32_t> lo_in(total), hi_in(total), t_lo(total), t_hi(total), lo(total), hi(total), st_in(n), st(n), t_sf(n), cur_a(n), cur_b(n);
    Arr<s5gpu_fit_t> fit1(n), t_fit(n), fit(n);
    if (!first.read(f) || !qlen.read(f) || !q0.read(f) || !ref.read(f) || !rows_in.read(f) || !lo_in.read(f) || !hi_in.read(f)) return -1;
    B.first = first.p; B.qlen = qlen.p; B.q0 = q0.p; B.ref = ref.p;
    std::vector<uint64_t> order;
    // s5gpu_path_fit_long_dev
    for (size_t k = 0; k < n; k++) st_in.p[k] = rows_in.p[k].status;
    fit_long(B, Pm, st_in.p, lo_in.p, hi_in.p, shuffle, verdict.p, P.p, order, fit1.p, st.p, q1.p);
    fit1.write(o); st.write(o); q1.write(o);
    // round 0: the fills, the verdicts of what came in, the copies
    q.fill(0); lo.fill(-1); hi.fill(-1);
    int32_t *cur_in = st_in.p, *cur_out = cur_a.p;
    verdicts(B, st_in.p, lo_in.p, hi_in.p, verdict.p, P.p, order, shuffle + 1u);
    for (uint32_t round = 0; round <= iters; round++) {
        if (round) {
            t_q.fill(0);
            fit_long(B, Pm, cur_in, lo.p, hi.p, shuffle + 2u * round, verdict.p, P.p, order, t_fit.p, t_sf.p, t_q.p);
            if (!t_rows.read(f) || !t_lo.read(f) || !t_hi.read(f)) return -1;
            t_fit.write(o); t_sf.write(o); t_q.write(o);
        }
        for (uint64_t x = 0; x < order.size(); x++) {
            const Seg sg = seg_of(B, P.p, order[x]);
            const uint32_t k = sg.k, r0 = sg.r0, r1 = sg.r1, v = verdict.p[k];
            if ((v & V_SKIPPED) || (round == 0 && v != V_USED)) continue;
            int32_t s;
            const int mode = long_round_rule(round, v, qlen.p[k], cur_in[k], round ? t_sf.p[k] : 0, round ? t_rows.p[k].status : 0, &s);
            if (mode == 0) continue;
            const uint64_t at = first.p[k];
            for (uint32_t i = r0; i < r1; i++) {
                int16_t qq = 0;
                int32_t l = -1, hh = -1;
                if (mode == 1) { qq = q0.p[at + i]; l = lo_in.p[at + i]; hh = hi_in.p[at + i]; }
                if (mode == 2) { qq = t_q.p[at + i]; l = t_lo.p[at + i]; hh = t_hi.p[at + i]; }
                q.p[at + i] = qq; lo.p[at + i] = l; hi.p[at + i] = hh;
            }
        }
        for (uint32_t k = 0; k < B.n; k++) {
            int32_t s;
            const int mode = long_round_rule(round, verdict.p[k], qlen.p[k], cur_in[k], round ? t_sf.p[k] : 0, round ? t_rows.p[k].status : 0, &s);
            if (round == 0 || cur_in[k] == 0) rows.p[k] = long_round_row(mode, s, round ? t_rows.p[k] : rows_in.p[k], rows.p[k]);
            if (mode == 2) { fit.p[k] = t_fit.p[k]; rounds.p[k] = round; }
            if (mode == 1 || mode == 3) { fit.p[k] = fit_none(); rounds.p[k] = 0; }
            cur_out[k] = s;
        }
        q.write(o); rows.write(o); lo.write(o); hi.write(o); fit.write(o); rounds.write(o);
        fwrite(cur_out, 4, n, o);
        cur_in = cur_out;
        cur_out = cur_out == cur_a.p ? cur_b.p : cur_a.p;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    for (;;) {
        const int rc = one_batch(f, o);
        if (rc < 0) return 1;
        if (rc > 0) break;
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def mixed_case(T, band, R, qs, seed, gap=None):
    """reads that track a reference of R levels, aligned by band_ref: -> (case, rows).  Every fifth read is tie-dense {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    queries, anchors = [], []
    for i, Q in enumerate(qs):
        s = int(rng.integers(0, R))
        cols = np.minimum(s + np.cumsum(rng.integers(0, 2, Q)), R - 1)
        if i % 5 == 4:
            q = rng.integers(-1, 2, Q).astype(np.int16)
        else:
            # the read's own units: the levels through 0.6 x - 9, so that a fit has something to find
            q = np.clip(np.rint(0.6 * ref[cols] - 9.0 + rng.normal(0.0, 2.0, Q)), -127, 127).astype(np.int16)
        queries.append(q)
        anchors.append((int(np.clip(s + rng.integers(-5, 6), 0, R - 1)), 0, R - 1)[i % 3])
    return er.banded_case(queries, ref, anchors, T, band, gap=gap, seed=seed)


def host_batches():
    """-> [(name, case, rows, T, band, S, P)]: every shape of SHAPES with every Q of QLENS against every R of RLENS at segments of 64 and 256
    (321 rows: six segments and two; 128: two and one), and the hand-made cases"""
    out = []
    for T, band in SHAPES:
        for n, R in enumerate(RLENS):
            case, rows = mixed_case(T, band, R, QLENS, 100 * T + band + R)
            for S in (64, 256):
                out.append(("shape %d %d R %d S %d" % (T, band, R, S), case, rows, T, band, S, params(min_cells=4, iters=1 + (n + S // 64) % 4)))
    for name, (case, rows, P) in hand_cases().items():
        out.append((name, case, rows, 64, 128, 64, P))
    return out


def write_host_batches(path, batches, shuffle=12345):
    traces = []
    with open(path, "wb") as fh:
        for name, case, rows, T, band, S, P in batches:
            t = []
            refine_long_ref(case, rows, T, band, P, trace=t)
            traces.append(t)
            fh.write(struct.pack("<IIIIQI", case.n, S, P["iters"], shuffle, case.total, case.R) + params_bytes(P))
            fh.write(case.first.astype("<u8").tobytes() + case.qlen.astype("<u4").tobytes() + case.q.tobytes() + case.ref.tobytes() + rows.tobytes())
            fh.write(case.lo.tobytes() + case.hi.tobytes())
            for r in t[1:]:
                fh.write(r["t_rows"].tobytes() + r["t_lo"].tobytes() + r["t_hi"].tobytes())
    return traces


def _build_host(tmp_path, extra=()):
    return host_build(tmp_path, "refine_long_host", REFINE_LONG_HOST, ["-O1", "-g", "-std=c++17", "-ffp-contract=off"], extra, api=True,
                      exe="refine_long_host" + ("_san" if extra else ""))


def _take(raw, at, dtype, count):
    a = np.frombuffer(raw, dtype, count, at)
    return a, at + a.nbytes


def _same_out(what, got, want):
    for key in ("q", "rows", "lo", "hi", "fit", "rounds"):
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), (what, key, got[key], want[key])


def _check_host_output(raw, batches, traces):
    at, kinds = 0, set()
    for (name, case, rows, T, band, S, P), t in zip(batches, traces):
        n, total = case.n, case.total
        wfit, wq1, wst = fit_long_ref(case, P, status=rows["status"].astype(np.int32))
        fit, at = _take(raw, at, FIT, n)
        st, at = _take(raw, at, np.int32, n)
        q1, at = _take(raw, at, np.int16, total)
        assert fit.tobytes() == wfit.tobytes() and st.tolist() == wst.tolist() and np.array_equal(q1, wq1), (name, fit, wfit, st, wst)
        kinds |= set(st.tolist())
        for j, r in enumerate(t):
            if j:
                tf, at = _take(raw, at, FIT, n)
                sf, at = _take(raw, at, np.int32, n)
                tq, at = _take(raw, at, np.int16, total)
                assert tf.tobytes() == r["fit"].tobytes() and sf.tolist() == r["sf"].tolist() and np.array_equal(tq, r["t_q"]), (name, j, tf, r["fit"], sf, r["sf"])
            got = {}
            for key, dt, cnt in (("q", np.int16, total), ("rows", EXT_ROW, n), ("lo", np.int32, total), ("hi", np.int32, total), ("fit", FIT, n),
                                 ("rounds", np.uint32, n), ("cur", np.int32, n)):
                got[key], at = _take(raw, at, dt, cnt)
            _same_out((name, j), got, r["out"])
            assert got["cur"].tolist() == r["cur"].tolist(), (name, j)
    assert at == len(raw)
    return kinds


def test_the_refine_long_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """seg_sums, sums_add, long_fit_status, long_round_rule, long_round_row of refine_dev.h behind long_verdict, seg_item (against seg_find
    and seg_next) and seg_rows_ok of ragged_dev.h, as g++ compiles them, on host_batches(): sums, fits, statuses, q' and the bookkeeping's outputs behind
    every round equal the restatement's byte for byte, whatever the segment size and the order of the segments; and the same program under
    ASan and UBSan, every array at exactly its size"""
    batches = host_batches()
    traces = write_host_batches(tmp_path / "in.bin", batches)
    exe = _build_host(tmp_path)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    kinds = _check_host_output((tmp_path / "out.bin").read_bytes(), batches, traces)
    assert {0, 7, PATH_ROW, FIT_FLAT, FIT_RANGE} <= kinds
    assert any(t[-1]["out"]["rounds"].max() >= 3 for t in traces) and any(len(set(t[-1]["out"]["rounds"].tolist())) > 1 for t in traces)
    # another order of the segments: the same bytes
    write_host_batches(tmp_path / "in2.bin", batches, shuffle=777)
    subprocess.check_call([exe, str(tmp_path / "in2.bin"), str(tmp_path / "out2.bin")])
    assert (tmp_path / "out2.bin").read_bytes() == (tmp_path / "out.bin").read_bytes()
    san = _build_host(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    p = subprocess.run([san, str(tmp_path / "in.bin"), str(tmp_path / "out_san.bin")], capture_output=True, text=True)
    assert p.returncode == 0 and not p.stderr.strip(), p.stderr[-2000:]
    assert (tmp_path / "out_san.bin").read_bytes() == (tmp_path / "out.bin").read_bytes()


# ---------------------------------------------------------------------------------------------------------------- the planted case

@pytest.mark.parametrize("T,band,n_events,R", PLANTED_SHAPES)
def test_the_planted_case(T, band, n_events, R):
    """§4.24's planted case in the restatement, seeds 1 .. 8, two rounds, the defaults.  For every seed: no read ends with a status, the share
    of events within 2 columns of the truth behind round 2 is at least the share before, and the cost does not grow.  For every seed whose
    first alignment mostly tracks (share before >= 0.873, the least the issue's prototype saw) the issue's floors: share >= 0.995 and final
    cost <= 0.2 of the first.
    What the restatement gives here (docs/codecs.md §4.24 has the lines): every seed but one clears the floors with 0.998 or better and at
    most 0.13 of the first cost; seed 3 at (64, 128) starts at 0.773, below anything the prototype saw -- the first band alignment has lost
    the read's head -- and goes to 0.841 with 0.35 of the cost: the rounds sharpen, they do not rescue."""
    for seed in PLANTED_SEEDS:
        q, ref, anchor, truth = er.planted_long(seed, n_events, R)
        case, rows = er.banded_case([q], ref, [anchor], T, band, gap=[0])
        t = []
        out = refine_long_ref(case, rows, T, band, params(), trace=t)
        before, after1, after = er.share_of(case.lo, case.hi, truth), er.share_of(t[1]["out"]["lo"], t[1]["out"]["hi"], truth), er.share_of(out["lo"], out["hi"], truth)
        c0, c1, c2 = int(rows[0]["cost"]), int(t[1]["out"]["rows"][0]["cost"]), int(out["rows"][0]["cost"])
        print("planted seed %d (%d, %d): share %.3f %.3f %.3f cost/event %.2f %.2f %.2f a, b %.2f %.1f then %.2f %.1f" % (
            seed, T, band, before, after1, after, c0 / n_events, c1 / n_events, c2 / n_events, t[1]["out"]["fit"][0]["a"], t[1]["out"]["fit"][0]["b"],
            out["fit"][0]["a"], out["fit"][0]["b"]))
        assert out["rows"][0]["status"] == 0 and out["rounds"][0] == 2, (seed, out["rows"][0])
        assert after >= before and c2 <= c0, (seed, before, after, c0, c2)
        if before >= PLANTED_TRACKS:
            assert after >= PLANTED_SHARE and c2 <= PLANTED_COST * c0, (seed, before, after, c0, c2)


def test_a_lost_alignment_terminates():
    """one seed of the 0.8 x + 20 case, where the first alignment is lost (share below 0.5): the rounds end, with a status the definition
    knows and as many rounds as it allows.  Nothing is asserted about improvement."""
    q, ref, anchor, truth = er.planted_long(1, 1500, 4096, 0.8, 20.0)
    case, rows = er.banded_case([q], ref, [anchor], 64, 128, gap=[0])
    assert er.share_of(case.lo, case.hi, truth) < 0.5
    out = refine_long_ref(case, rows, 64, 128, params())
    assert out["rows"][0]["status"] in (0, FIT_FLAT, FIT_RANGE, PATH_ROW) and 0 <= out["rounds"][0] <= 2


# ---------------------------------------------------------------------------------------------------------------- arguments, exports

def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3): the pointers are never dereferenced on the host, so made-up aligned addresses serve"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    A = 1 << 20
    nan, inf = float("nan"), float("inf")
    bad_refine = [dict(a_min=0.0), dict(a_min=3.0), dict(a_max=inf), dict(a_min=nan), dict(b_max=-1.0), dict(b_max=nan), dict(clip=0), dict(clip=32768),
                  dict(pad=65536), dict(min_cells=1), dict(iters=0), dict(iters=5)]
    bad_band = [dict(emin=0), dict(emax=(1 << 20) + 1), dict(tile_rows=32), dict(tile_rows=192), dict(band=96), dict(band=4160), dict(clip=0), dict(scale=nan)]

    wb = L.s5gpu_path_fit_long_work_bytes
    assert wb(4, (1 << 40) + 1) == 0 and wb(4, 1000) == L.s5gpu_pileup_long_work_bytes(4, 1000) + 48 * 4 and wb(0, 0) > 0
    wr = L.s5gpu_extend_refine_work_bytes
    assert wr(4, (1 << 40) + 1) == 0 and wr(4, 1000) == wb(4, 1000) + 4 * (32 + 64) + 3 * 16 + 2 * 4000 + 2000

    def fl(n=4, q=A, first=A, qlen=A, total=1000, ref=A, R=100, lo=A, hi=A, si=A, P=None, pnull=False, work=A, wbytes=1 << 30, fit=A, qo=A + 4096, so=A + 8192):
        p = c_params(P or params())
        return L.s5gpu_path_fit_long_dev(n, q, first, qlen, total, ref, R, lo, hi, si, None if pnull else C.byref(p), work, wbytes, fit, qo, so, None)
    assert fl(pnull=True) == -1 and fl(R=0) == -1 and fl(R=1 << 31) == -1 and fl(ref=None) == -1 and fl(total=(1 << 40) + 1) == -1
    for kw in bad_refine:
        assert fl(P=params(**kw)) == -1, kw
    for name in ("q", "first", "qlen", "lo", "hi", "si", "work", "fit", "so"):
        assert fl(**{name: None}) == -1, name
    assert fl(q=A + 1) == -1 and fl(first=A + 4) == -1 and fl(qlen=A + 2) == -1 and fl(ref=A + 1) == -1 and fl(lo=A + 2) == -1 and fl(hi=A + 2) == -1
    assert fl(si=A + 2) == -1 and fl(work=A + 8) == -1 and fl(fit=A + 8) == -1 and fl(qo=A + 1) == -1 and fl(so=A + 2) == -1
    assert fl(qo=A) == -1 and fl(so=A, si=A) == -1                         # an output that is an input
    assert fl(wbytes=wb(4, 1000) - 1) == -3 and fl(wbytes=0) == -3
    assert fl(n=0) == 0 and fl(n=0, q=None, fit=None, work=None, wbytes=0) == 0

    slot = L.s5gpu_sdtw_path_slot_bytes(256, 512)
    need = L.s5gpu_sdtw_band_scratch_bytes(4, 1000, 256, 512)

    def rf(n=4, q=A, first=A, qlen=A, total=1000, ref=A, R=100, ri=A, li=A, hi_=A, BP=None, bnull=False, P=None, pnull=False, scratch=A, sbytes=1 << 30, work=A,
           wbytes=1 << 30, qo=A + 4096, ro=A + 4096, lo=A + 4096, ho=A + 4096, fit=A, rnd=A):
        p, bp = c_params(P or params()), BP or bparams()
        return L.s5gpu_extend_refine_dev(n, q, first, qlen, total, ref, R, ri, li, hi_, None if bnull else C.byref(bp), None if pnull else C.byref(p), scratch,
                                         sbytes, work, wbytes, qo, ro, lo, ho, fit, rnd, None)
    assert rf(pnull=True) == -1 and rf(bnull=True) == -1 and rf(R=0) == -1 and rf(R=1 << 31) == -1 and rf(ref=None) == -1 and rf(total=(1 << 40) + 1) == -1
    for kw in bad_refine:
        assert rf(P=params(**kw)) == -1, kw
    for kw in bad_band:
        assert rf(BP=bparams(**kw)) == -1, kw
    for name in ("q", "first", "qlen", "ri", "li", "hi_", "scratch", "work", "qo", "ro", "lo", "ho", "fit", "rnd"):
        assert rf(**{name: None}) == -1, name
    for name, off in (("q", 1), ("first", 4), ("qlen", 2), ("ref", 1), ("ri", 8), ("li", 2), ("hi_", 2), ("scratch", 8), ("work", 8), ("qo", 1), ("ro", 8),
                      ("lo", 2), ("ho", 2), ("fit", 8), ("rnd", 2)):
        assert rf(**{name: (A + 4096 if name in ("qo", "ro", "lo", "ho") else A) + off}) == -1, name
    assert rf(qo=A) == -1 and rf(ro=A) == -1 and rf(lo=A) == -1 and rf(ho=A) == -1                  # an output that is an input
    assert rf(sbytes=need - 1) == -3 and rf(sbytes=need - slot) == -3 and rf(sbytes=0) == -3 and rf(wbytes=wr(4, 1000) - 1) == -3
    assert rf(n=0) == 0 and rf(n=0, sbytes=0, wbytes=0, q=None, ro=None) == 0

    # the batch call: the cases of s5gpu_extend_batch, the refine parameters, the new outputs
    vp = C.c_void_p
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    bufs = dict(map=np.full(16, 0xA5, np.uint8), rows1=np.full(32, 0xA5, np.uint8), rows=np.full(32, 0xA5, np.uint8), first=np.full(2, 77, np.uint64),
                lo=np.full(64, -7, np.int32), hi=np.full(64, -7, np.int32), q=np.full(64, -7, np.int16), fit=np.full(64, 0xA5, np.uint8),
                rnd=np.full(1, 77, np.uint32), st=np.full(1, -7, np.int32))
    before = {k: v.copy() for k, v in bufs.items()}

    def batch(pr=(0, 64, 10, 32.0, 127, 1), BP=None, bnull=False, P=None, pnull=False, R=100, ref=True, methods=(1, 1), **off):
        e, p, bp, rp = _lib.EventParams(*DNA), _lib.MapParams(*pr), BP or bparams(emin=10), c_params(P or params())
        a = {k: (None if off.get(k) is False else v.ctypes.data_as(vp)) for k, v in bufs.items()}
        return L.s5gpu_extend_refine_batch(1, rec_p, rl, methods[0], methods[1], C.byref(e), C.byref(p), None if bnull else C.byref(bp),
                                           None if pnull else C.byref(rp), 0, h_ref.ctypes.data_as(vp) if ref else None, R, a["map"], a["rows1"], a["rows"],
                                           a["first"], a["lo"], a["hi"], None, a["q"], 64, a["fit"], a["rnd"], a["st"])
    assert batch(pr=(0, 0, 1, 32.0, 127, 1)) == -1 and batch(R=0) == -1 and batch(ref=False) == -1 and batch(bnull=True) == -1 and batch(pnull=True) == -1
    assert batch(methods=(9, 1)) == -1
    for name in ("map", "rows1", "rows", "first", "lo", "fit"):
        assert batch(**{name: False}) == -1, name
    for kw in bad_refine:
        assert batch(P=params(**kw)) == -1, kw
    for kw in bad_band:
        assert batch(BP=bparams(**dict(dict(emin=10), **kw))) == -1, kw
    assert batch(BP=bparams(emin=10, skip=1)) == -1
    assert all((bufs[k] == before[k]).all() for k in bufs)
    # the switches of the handles: a NULL handle
    p = c_params(params())
    assert L.s5gpu_pileup_set_refine(None, C.byref(p)) == -1 and L.s5gpu_contrast_set_refine(None, C.byref(p)) == -1


def test_library_exports_the_whole_read_refine_calls_and_the_tools_take_the_flag():
    """the symbols are in the header, in the library and in the bindings' list; s5extend, s5pileup and s5contrast know --refine"""
    from slow5tools_amd import _lib, build, contrast, extend, pileup

    build.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "slow5gpu.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_CALLS:
        assert hasattr(L, name) and name in _lib.EXPORTS and name + "(" in hdr and name in exported, name
    for bad in (0, 64, -1):
        assert L.s5gpu_set_option(b"refine_long_passes", bad) == -1
    assert L.s5gpu_set_option(b"refine_long_passes", 63) == 0
    for exe in (extend.S5EXTEND, pileup.S5PILEUP, contrast.S5CONTRAST):
        p = subprocess.run([exe, "--refine", "--iters", "9"], capture_output=True, text=True)
        assert p.returncode == 2 and "iters" in p.stderr, (exe, p.stderr)                          # the flag is known, its value refused
        p = subprocess.run([exe, "--refine", "--slope", "2,1"], capture_output=True, text=True)
        assert p.returncode == 2 and "slope" in p.stderr, (exe, p.stderr)
    assert extend.EXTEND_REFINE_LINE.names[-7:] == ("scale", "shift", "rounds", "cost_refined", "ref_start_refined", "ref_end_refined", "fit")


# ---------------------------------------------------------------------------------------------------------------- gpu

def _options(env, seg=DEFAULT_SEG, sort=DEFAULT_SORT, grid=DEFAULT_GRID):
    for key, v in ((b"pileup_long_seg", seg), (b"pileup_long_sort", sort), (b"pileup_long_grid", grid)):
        env.lib.check(env.L.s5gpu_set_option(key, v), key.decode())


def _upload(env, case):
    return dict(q=to_dev(env, case.q), first=to_dev(env, case.first.view(np.int64)), qlen=to_dev(env, case.qlen.view(np.int32)), ref=to_dev(env, case.ref),
                lo=to_dev(env, case.lo), hi=to_dev(env, case.hi), status=to_dev(env, case.status))


def _fit(env, d, P, want_queries=True):
    fit, q1, st = env.extend.fit_long_dev(d["q"], d["first"], d["qlen"], d["ref"], d["lo"], d["hi"], d["status"], c_params(P), want_queries)
    env.torch.cuda.synchronize()
    return fit.cpu().numpy().view(FIT).reshape(-1), (q1.cpu().numpy() if want_queries else None), st.cpu().numpy()


def _same_fit(what, got, want):
    assert got[0].tobytes() == want[0].tobytes(), (what, got[0], want[0])
    assert got[2].tolist() == want[2].tolist(), (what, got[2], want[2])
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), what


def _band_on_device(env, qs, ref, anchors, T, band, gap=None, seed=0):
    """the layout of er.banded_case, the paths from band_dev (which test_extend.py holds against band_ref) -> (case, rows)"""
    ex = env.extend
    rng = np.random.default_rng(seed)
    gap = [int(x) for x in (rng.integers(0, 3, len(qs)) if gap is None else gap)]
    first = np.concatenate(([0], np.cumsum([len(q) + g for q, g in zip(qs, gap)]))).astype(np.uint64)
    q = np.zeros(int(first[-1]), np.int16)
    for k, x in enumerate(qs):
        q[int(first[k]):int(first[k]) + len(x)] = x
    p = ex.BandParams(0, 1, 1 << 20, T, band)
    rows, lo, hi = ex.band_dev(to_dev(env, q), to_dev(env, first.view(np.int64)), to_dev(env, np.array([len(x) for x in qs], np.int32)), to_dev(env, ref),
                               to_dev(env, np.array(anchors, np.int32)), None, p)
    env.torch.cuda.synchronize()
    rows = rows.cpu().numpy().view(EXT_ROW).reshape(-1).copy()
    return LongCase(q, first, [len(x) for x in qs], ref, lo.cpu().numpy(), hi.cpu().numpy(), rows["status"].astype(np.int32)), rows


def _flawed(case, rows):
    """the mixed batch with its flaws: read 3 comes in with a status, read 8 (321 rows) has a broken row in its first segment and read 17 (321
    rows) one in its last, and the last read's rows end beyond the arrays"""
    case = case.copy()
    rows = rows.copy()
    assert case.qlen[8] == 321 and case.qlen[17] == 321 and case.qlen[3] == 65 and case.qlen[case.n - 1] == 70
    case.status[3], rows["status"][3] = 7, 7
    f8, f17 = int(case.first[8]), int(case.first[17])
    case.lo[f8 + 5] = case.hi[f8 + 5] + 1                                   # lo > hi
    case.hi[f17 + 318] += 2                                                 # row 319 no longer begins where row 318 ended
    case.first[case.n] = case.total + 5
    return case, rows


@pytest.mark.gpu
@pytest.mark.parametrize("R", [65, 300])
def test_fit_long_is_exact_on_a_mixed_batch(gpu, R):
    """s5gpu_path_fit_long_dev on 40 ragged reads (every Q of QLENS four times, two reads without a query, 5 and 70 rows) whose paths come from
    band_dev at (64, 128), with a read that comes in with a status, broken rows in a first and in a last segment and a `first` out of
    range: fits, sums, statuses and q' equal fit_long_ref, the same bytes at segments of 64 and 256 with the sort on and off, at segments
    of 64 with one workgroup (each of its four waves walks some thirty consecutive segments across the reads' boundaries, the flawed reads
    among them: the sums held and flushed, the read carried from segment to segment) and with three (most of the twelve waves have a short
    slice or none), with and without queries_out, and on two streams into separate outputs"""
    t = gpu.torch
    rng = np.random.default_rng(4240 + R)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    qs, anchors = [], []
    for i, Q in enumerate(MIXED_Q):
        s = int(rng.integers(0, R))
        cols = np.minimum(s + np.cumsum(rng.integers(0, 2, Q)), R - 1)
        qs.append(rng.integers(-1, 2, Q).astype(np.int16) if i % 5 == 4 else
                  np.clip(np.rint(0.6 * ref[cols] - 9.0 + rng.normal(0.0, 2.0, Q)), -127, 127).astype(np.int16))
        anchors.append((int(np.clip(s + rng.integers(-5, 6), 0, R - 1)), 0, R - 1)[i % 3])
    case, rows = _flawed(*_band_on_device(gpu, qs, ref, anchors, 64, 128, seed=R))
    P = params(min_cells=16)
    want = fit_long_ref(case, P)
    assert want[2][3] == 7 and want[2][8] == PATH_ROW and want[2][17] == PATH_ROW and want[2][case.n - 1] == PATH_ROW and want[2][36] == 0
    assert {0, FIT_FLAT} <= set(want[2].tolist()) and (want[2] == 0).sum() >= 10
    d = _upload(gpu, case)
    try:
        for seg in (64, 256):
            for sort in (1, 0):
                _options(gpu, seg=seg, sort=sort)
                _same_fit((R, seg, sort), _fit(gpu, d, P), want)
        for grid in (1, 3):
            _options(gpu, seg=64, grid=grid)
            _same_fit((R, "grid", grid), _fit(gpu, d, P), want)
        _options(gpu, seg=256, sort=0)
        _same_fit((R, "no queries"), _fit(gpu, d, P, want_queries=False), want)
    finally:
        _options(gpu)
    s1, s2 = t.cuda.Stream(), t.cuda.Stream()
    P2 = params(min_cells=2, a_max=1.5)
    want2 = fit_long_ref(case, P2)
    with t.cuda.stream(s1):
        a = gpu.extend.fit_long_dev(d["q"], d["first"], d["qlen"], d["ref"], d["lo"], d["hi"], d["status"], c_params(P))
    with t.cuda.stream(s2):
        b = gpu.extend.fit_long_dev(d["q"], d["first"], d["qlen"], d["ref"], d["lo"], d["hi"], d["status"], c_params(P2))
    t.cuda.synchronize()
    for got, w in ((a, want), (b, want2)):
        _same_fit((R, "streams"), (got[0].cpu().numpy().view(FIT).reshape(-1), got[1].cpu().numpy(), got[2].cpu().numpy()), w)
    for key, arr in (("q", case.q), ("lo", case.lo), ("hi", case.hi)):
        assert np.array_equal(d[key].cpu().numpy(), arr), "an input was written"


@pytest.mark.gpu
def test_fit_long_over_many_workgroups_and_a_long_read(gpu):
    """300 reads of 65 .. 129 rows, and a read of 20 000 rows that tracks its reference among short ones: 79 segments of 256 rows whose sums
    meet in one read's six words"""
    rng = np.random.default_rng(77)
    R = 300
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    qs, anchors = [], []
    for i in range(300):
        Q = 65 + i % 65
        s = int(rng.integers(0, R))
        cols = np.minimum(s + np.cumsum(rng.integers(0, 2, Q)), R - 1)
        qs.append(np.clip(np.rint(0.8 * ref[cols] + 6.0 + rng.normal(0.0, 2.0, Q)), -127, 127).astype(np.int16))
        anchors.append(s)
    case, _ = _band_on_device(gpu, qs, ref, anchors, 64, 128, seed=1)
    P = params()
    _same_fit("300 reads", _fit(gpu, _upload(gpu, case), P), fit_long_ref(case, P))
    q, ref, anchor = tracking_read(rng, 20000, 24000)
    short = [tracking_read(np.random.default_rng(k), 90, 24000)[0] for k in range(4)]
    case, rows = _band_on_device(gpu, short[:2] + [q] + short[2:], ref, [5, 9, anchor, 100, 200], 64, 128, seed=2)
    assert rows["status"].tolist() == [0] * 5 and rows["qlen"][2] == 20000
    want = fit_long_ref(case, P)
    assert want[2][2] == 0 and want[0][2]["n"] >= 20000
    _same_fit("a long read", _fit(gpu, _upload(gpu, case), P), want)


def _refine(env, case, rows, T, band, P, scratch_bytes_=None):
    d = _upload(env, case)
    x = env.extend.refine_long_dev(d["q"], d["first"], d["qlen"], d["ref"], to_dev(env, rows.view(np.int64).reshape(-1, 4)), d["lo"], d["hi"],
                                   env.extend.BandParams(0, 1, 1 << 20, T, band), c_params(P), scratch_bytes_)
    env.torch.cuda.synchronize()
    return dict(q=x.queries.cpu().numpy(), rows=x.rows.cpu().numpy().view(EXT_ROW).reshape(-1), lo=x.lo.cpu().numpy(), hi=x.hi.cpu().numpy(),
                fit=x.fit.cpu().numpy().view(FIT).reshape(-1), rounds=x.rounds.cpu().numpy().view(np.uint32))


_PLANTED = {}


def planted_batch():
    """the eight planted reads of 1500 events and the lost one (0.8 x + 20) in one batch against their references laid end to end, aligned by
    band_ref at (64, 128), and the trace of four rounds -> (case, rows, trace)"""
    if not _PLANTED:
        reads = [er.planted_long(seed, 1500, 4096) for seed in PLANTED_SEEDS] + [er.planted_long(1, 1500, 4096, 0.8, 20.0)]
        ref = np.concatenate([r[1] for r in reads])
        case, rows = er.banded_case([r[0] for r in reads], ref, [r[2] + 4096 * k for k, r in enumerate(reads)], 64, 128, seed=9)
        t = []
        refine_long_ref(case, rows, 64, 128, params(iters=4), trace=t)
        _PLANTED["x"] = (case, rows, t)
    return _PLANTED["x"]


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 4])
def test_the_rounds_equal_the_restatement_on_the_planted_reads(gpu, iters):
    """s5gpu_extend_refine_dev on the planted reads and the lost one: q', rows, lo, hi, fits, statuses and rounds equal refine_long_ref's
    behind `iters` rounds"""
    case, rows, t = planted_batch()
    got = _refine(gpu, case, rows, 64, 128, params(iters=iters))
    _same_out(("planted", iters), got, t[iters]["out"])
    assert (got["rounds"] <= iters).all() and got["rounds"].max() == iters


@pytest.mark.gpu
def test_the_rounds_on_a_mixed_batch_where_reads_drop_out(gpu):
    """the mixed batch with its flaws through four rounds with a slope limit that some reads meet in one round and others in a later one:
    everything equals refine_long_ref, also at segments of 64 without the sort, and there with one workgroup and with three (see
    test_fit_long_is_exact_on_a_mixed_batch); and a scratch one slot too small is refused with nothing written"""
    t = gpu.torch
    case, rows = mixed_case(64, 128, 300, MIXED_Q, 4241)
    case, rows = _flawed(case, rows)
    P = params(iters=4, min_cells=16, a_max=1.6)
    want = refine_long_ref(case, rows, 64, 128, P)
    print("rounds", want["rounds"].tolist(), "statuses", want["rows"]["status"].tolist())
    assert want["rows"]["status"][[3, 8, 17, case.n - 1]].tolist() == [7, PATH_ROW, PATH_ROW, PATH_ROW]
    assert len(set(want["rounds"].tolist())) >= 3 and {0, FIT_RANGE, FIT_FLAT} <= set(want["rows"]["status"].tolist())
    _same_out("mixed", _refine(gpu, case, rows, 64, 128, P), want)
    try:
        _options(gpu, seg=64, sort=0)
        _same_out("mixed, segments of 64", _refine(gpu, case, rows, 64, 128, P), want)
        for grid in (1, 3):
            _options(gpu, seg=64, grid=grid)
            _same_out(("mixed, segments of 64, grid", grid), _refine(gpu, case, rows, 64, 128, P), want)
    finally:
        _options(gpu)
    # a scratch one slot too small
    ex = gpu.extend
    d = _upload(gpu, case)
    need, slot = ex.scratch_bytes(case.n, case.total, 64, 128), gpu.L.s5gpu_sdtw_path_slot_bytes(64, 128)
    wb = gpu.L.s5gpu_extend_refine_work_bytes(case.n, case.total)
    g = lambda count, dt: t.full((count,), -3, dtype=dt, device="cuda")
    scratch, work = g(need // 4, t.int32), g(wb // 4 + 4, t.int32)
    out = [g(case.total, t.int16), g(case.n * 4, t.int64), g(case.total, t.int32), g(case.total, t.int32), g(case.n * 8, t.int64), g(case.n, t.int32)]
    d_rows = to_dev(gpu, rows.view(np.int64).reshape(-1, 4))
    bp, rp = ex.BandParams(0, 1, 1 << 20, 64, 128), c_params(P)
    rc = gpu.L.s5gpu_extend_refine_dev(case.n, d["q"].data_ptr(), d["first"].data_ptr(), d["qlen"].data_ptr(), case.total, d["ref"].data_ptr(), case.R,
                                       d_rows.data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(), C.byref(bp), C.byref(rp), scratch.data_ptr(), need - slot,
                                       work.data_ptr(), wb, *[o.data_ptr() for o in out], None)
    t.cuda.synchronize()
    assert rc == -3 and b"scratch" in gpu.L.s5gpu_last_error()
    assert all(bool((o == -3).all()) for o in out + [scratch, work])
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-3"):
        _refine(gpu, case, rows, 64, 128, P, scratch_bytes_=need - 1)


@pytest.fixture(scope="module")
def chain(gpu):
    """two small synthetic files as test_contrast makes them (a read a side too short for a query); a reference that holds the levels of
    three of the reads, squeezed to 0.7 x + 180 so that they sit higher and closer together than the reads have them; and what the
    unrefined device chain leaves for each side as a LongCase"""
    rng = np.random.default_rng(4024)
    sigs = [[levels_signal(n, rng) for n in lengths] for lengths in ([30000, 100, 26000, 28000], [27000, 31000, 100])]
    sigs[1][0] = sigs[0][0]                                                # a read both sides hold: their columns overlap
    recs = [[record(10 * s + i, sig) for i, sig in enumerate(side)] for s, side in enumerate(sigs)]
    kw = dict(skip=2, qmax=100, qmin=20, tile_rows=64, band=128)
    env = type("Chain", (), {})()
    env.decs = [gpu.press.decode_to_device(r) for r in recs]
    means = []
    for dec in env.decs:
        ev, first = gpu.events.events_dev(dec, DNA, "raw")
        h_ev, h_first = ev.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
        means.append([h_ev["mean"][h_first[i]:h_first[i + 1]] for i in range(len(h_first) - 1)])
    squeeze = lambda m: (0.7 * m.astype(np.float64) + 180.0).astype(np.float32)
    levels = np.concatenate([rng.normal(500.0, 110.0, 300), squeeze(means[0][0]), rng.normal(500.0, 110.0, 200), squeeze(means[0][3]),
                             rng.normal(500.0, 110.0, 100), squeeze(means[1][1]), rng.normal(500.0, 110.0, 100)]).astype(np.float32)
    ref = quant_ref(levels)
    env.recs, env.levels, env.ref, env.kw, env.P = recs, levels, ref, kw, params(min_cells=16, iters=2)
    env.cases, env.rows, env.maps, env.wants = [], [], [], []
    for dec in env.decs:
        ev, first = gpu.events.events_dev(dec, DNA, "raw")
        out, x = gpu.extend.extend_dev(dec, ref, host=False, **kw)
        rows = x.rows.cpu().numpy().view(EXT_ROW).reshape(-1).copy()
        case = LongCase(x.queries.cpu().numpy(), x.first.cpu().numpy().astype(np.uint64), x.qlen.cpu().numpy(), ref, x.lo.cpu().numpy(), x.hi.cpu().numpy(),
                        rows["status"], ev.cpu().numpy().view(EVENT).reshape(-1), kw["skip"])
        env.cases.append(case)
        env.rows.append(rows)
        env.maps.append(out.cpu().numpy())
        env.wants.append(refine_long_ref(case, rows, kw["tile_rows"], kw["band"], env.P))
    return env


def _ragged(first, arr):
    return [arr[int(first[i]):int(first[i + 1])] for i in range(len(first) - 1)]


@pytest.mark.gpu
def test_the_chain_with_refine(gpu, chain, tmp_path):
    """extend_dev(refine=P) equals the restatement fed with what the unrefined chain leaves; read_extend(refine=P) equals it, also with a
    scratch_max that forces several groups; s5extend --refine prints those rows; and refine=None is what it was"""
    ex = gpu.extend
    kw, P = chain.kw, chain.P
    rp = c_params(P)
    case, rows, want = chain.cases[0], chain.rows[0], chain.wants[0]
    print("chain: statuses", want["rows"]["status"].tolist(), "rounds", want["rounds"].tolist(), "fits", want["fit"]["a"].tolist(), want["fit"]["b"].tolist())
    assert rows["status"].tolist() == [0, QUERY_SHORT, 0, 0] and want["rows"]["status"][[0, 3]].tolist() == [0, 0] and want["rounds"][[0, 1, 3]].tolist() == [2, 0, 2]
    mrows, X = ex.extend_dev(chain.decs[0], chain.ref, refine=rp, **kw)
    got = dict(q=X.queries, rows=X.rows, lo=X.lo, hi=X.hi, fit=X.fit, rounds=X.rounds.view(np.uint32))
    _same_out("extend_dev", got, want)
    assert X.rows_first.tolist() == rows.tolist() and not np.array_equal(X.lo, case.lo)
    m0, X0 = ex.extend_dev(chain.decs[0], chain.ref, refine=None, **kw)
    assert not hasattr(X0, "fit") and X0.rows.tolist() == rows.tolist() and np.array_equal(X0.lo, case.lo) and np.array_equal(X0.queries, case.q)
    # the batch call, in one group and in several
    E = np.diff(case.first.astype(np.int64))
    plain = ex.read_extend(chain.recs[0], chain.ref, **kw)
    assert plain[1].tolist() == rows.tolist() and len(plain) == 7
    for smax in (0, ex.scratch_bytes(1, int(E.max()), kw["tile_rows"], kw["band"])):
        b = ex.read_extend(chain.recs[0], chain.ref, scratch_max=smax, refine=rp, **kw)
        b_map, b_rows, b_first, b_lo, b_hi, b_ev, b_st, b_rows1, b_q, b_fit, b_rounds = b
        assert b_rows.tolist() == want["rows"].tolist() and b_rows1.tolist() == rows.tolist() and b_fit.tobytes() == want["fit"].tobytes(), smax
        assert b_rounds.tolist() == want["rounds"].tolist() and b_st.tolist() == want["rows"]["status"].tolist() and b_map.tolist() == plain[0].tolist()
        assert b_first.tolist() == np.concatenate([[0], np.cumsum(b_rows["qlen"])]).tolist()
        for i, (lo, hi, q, ev) in enumerate(zip(_ragged(b_first, b_lo), _ragged(b_first, b_hi), _ragged(b_first, b_q), _ragged(b_first, b_ev))):
            f0, Q = int(case.first[i]), int(b_rows["qlen"][i])
            assert np.array_equal(lo, want["lo"][f0:f0 + Q]) and np.array_equal(hi, want["hi"][f0:f0 + Q]) and np.array_equal(q, want["q"][f0:f0 + Q]), (smax, i)
            assert ev.tobytes() == case.ev[f0 + kw["skip"]:f0 + kw["skip"] + Q].tobytes(), (smax, i)
    # the tool
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("".join("%.9g\n" % v for v in chain.levels))
    synth_file(tmp_path / "reads.blow5", chain.recs[0])
    ids = [ob_id(10 * 0 + i) for i in range(4)]
    args = ["--skip", str(kw["skip"]), "--events", str(kw["qmax"]), "--min-events", str(kw["qmin"]), "--tile", str(kw["tile_rows"]), "--band", str(kw["band"]),
            str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([ex.S5EXTEND, "-K", "3", "--refine"] + args, capture_output=True, timeout=120)
    assert p.returncode == 0 and b"short" in p.stderr, p.stderr
    lines = []
    how = {0: b"ok", FIT_FLAT: b"flat", FIT_RANGE: b"range", PATH_ROW: b"row"}
    for i in range(4):
        if rows[i]["status"]:
            lines.append(ids[i] + b"\t*" * 14 + b"\n")
            continue
        r1, r2, f = rows[i], want["rows"][i], want["fit"][i]
        lines.append(b"%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
            ids[i], r1["qlen"], r1["cost"], b"%.3f" % (int(r1["cost"]) / int(r1["qlen"])), r1["start"], r1["end"], r1["tiles"], chain.maps[0][i][2],
            b"%.9g" % f["a"], b"%.9g" % f["b"], want["rounds"][i], r2["cost"], r2["start"], r2["end"], how[int(r2["status"])]))
    assert p.stdout == b"".join(lines), (p.stdout[:300], lines[0])
    fids, fl = ex.file_extend(tmp_path / "reads.blow5", ref_txt, batch=3, refine=True, **kw)
    assert fids == ids and fl["cost_refined"].tolist() == [int(r["cost"]) if r["qlen"] else -1 for r in want["rows"]] and fl["fit"].tolist()[0] == b"ok"
    p1 = subprocess.run([ex.S5EXTEND, "-K", "3"] + args, capture_output=True, timeout=120)
    assert p1.returncode == 0 and [l.split(b"\t")[:8] for l in p1.stdout.splitlines()] == [l.split(b"\t")[:8] for l in p.stdout.splitlines()]
    # --per-event lines come from the refined path
    p = subprocess.run([ex.S5EXTEND, "--refine", "--per-event"] + args, capture_output=True, timeout=120)
    got_lo = [int(l.split(b"\t")[5]) for l in p.stdout.splitlines() if l.startswith(ids[0] + b"\t")]
    assert p.returncode == 0 and got_lo == want["lo"][int(case.first[0]):int(case.first[0]) + int(rows[0]["qlen"])].tolist()


def ob_id(i):
    x = ob.synth_read_id(i)
    return x if isinstance(x, bytes) else x.encode()


@pytest.mark.gpu
def test_pileup_and_contrast_with_refine(gpu, chain, tmp_path):
    """pileup_whole_dev(refine=P), PileupWhole(refine=P) and s5pileup --whole --refine give the table of pileup_long_ref fed with
    refine_long_ref's outputs; contrast_whole_dev(refine=P), Contrast(refine=P) and s5contrast --refine the rows of contrast_ref on hist_ref
    of the same; without refine everything is what it was; set_refine is refused once a batch has been added"""
    pl, ct = gpu.pileup, gpu.contrast
    kw, P = chain.kw, chain.P
    rp = c_params(P)
    R = len(chain.ref)
    fed = [er.refined_case(c, w) for c, w in zip(chain.cases, chain.wants)]
    tables = [table_bytes(pileup_long_ref(c)) for c in fed]
    plain = [table_bytes(pileup_long_ref(c)) for c in chain.cases]
    assert tables[0] != plain[0] and tables[1] != plain[1]
    hists = [cr.hist_ref(c) for c in fed]
    for s in (0, 1):
        acc, st, ext = pl.pileup_whole_dev(chain.decs[s], chain.ref, pl.new_acc(R), refine=rp, **kw)
        assert table_bytes(pl.to_host(acc)) == tables[s] and st.cpu().numpy().tolist() == chain.wants[s]["rows"]["status"].tolist()
        assert ext.cpu().numpy().view(EXT_ROW).reshape(-1).tolist() == chain.wants[s]["rows"].tolist()
        acc, st, ext = pl.pileup_whole_dev(chain.decs[s], chain.ref, pl.new_acc(R), refine=None, **kw)
        assert table_bytes(pl.to_host(acc)) == plain[s]
        with pl.PileupWhole(chain.ref, refine=rp, **kw) as h:
            rc, map_rows, rows, status = h.add(chain.recs[s][:2])
            assert gpu.L.s5gpu_pileup_set_refine(h._h, None) == -1          # a batch has been added
            h.add(chain.recs[s][2:])
            assert rc == 0 and rows.tolist() == chain.wants[s]["rows"][:2].tolist()
            assert table_bytes(h.close()) == tables[s]
        with pl.PileupWhole(chain.ref, refine=None, **kw) as h:
            h.add(chain.recs[s])
            assert table_bytes(h.close()) == plain[s]
    f = pl.Pileup(chain.ref, skip=2, qmax=100, qmin=20)
    assert gpu.L.s5gpu_pileup_set_refine(f._h, C.byref(rp)) == -1          # not a whole-read handle
    f.abandon()
    # contrast
    want_rows = cr.contrast_ref(hists[0][1], hists[1][1], pileup_long_ref(fed[0])[1], pileup_long_ref(fed[1])[1])
    rows, accs, hs = ct.contrast_whole_dev(chain.decs[0], chain.decs[1], chain.ref, refine=rp, **kw)
    rows = ct.rows_to_host(rows)
    assert rows.tobytes() == np.ascontiguousarray(want_rows).tobytes()
    for s in (0, 1):
        head, counts = ct.hist_to_host(hs[s])
        assert cr.hist_bytes_of((head, counts)) == cr.hist_bytes_of(hists[s]) and table_bytes(pl.to_host(accs[s])) == tables[s]
    with ct.Contrast(chain.ref, refine=rp, **kw) as h:
        for s in (1, 0):
            h.add(s, chain.recs[s])
        assert gpu.L.s5gpu_contrast_set_refine(h._h, None) == -1
        hrows, a, b = h.close()
    assert hrows.tobytes() == rows.tobytes() and [table_bytes(a), table_bytes(b)] == tables
    rows0, _, _ = ct.contrast_whole_dev(chain.decs[0], chain.decs[1], chain.ref, **kw)
    with ct.Contrast(chain.ref, refine=None, **kw) as h:
        for s in (0, 1):
            h.add(s, chain.recs[s])
        hrows0, a, b = h.close()
    assert hrows0.tobytes() == ct.rows_to_host(rows0).tobytes() and [table_bytes(a), table_bytes(b)] == plain
    # the tools
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("".join("%.9g\n" % v for v in chain.levels))
    for s, name in enumerate(("a.blow5", "b.blow5")):
        synth_file(tmp_path / name, chain.recs[s])
    args = ["--skip", str(kw["skip"]), "--events", str(kw["qmax"]), "--min-events", str(kw["qmin"]), "--tile", str(kw["tile_rows"]), "--band", str(kw["band"])]
    paths = [str(ref_txt), str(tmp_path / "a.blow5"), str(tmp_path / "b.blow5")]
    p = subprocess.run([pl.S5PILEUP, "-K", "3", "--whole", "--refine"] + args + paths[:2], capture_output=True, timeout=120)
    cols = pileup_long_ref(fed[0])[1]
    refused = [int(np.isin(w["rows"]["status"], (FIT_FLAT, FIT_RANGE)).sum()) for w in chain.wants]
    assert p.returncode == 0 and b"reads refused by the fit %d" % refused[0] in p.stderr and p.stdout == b"".join(pile_lines(chain.ref, cols)), p.stderr
    p = subprocess.run([pl.S5PILEUP, "-K", "3", "--whole"] + args + paths[:2], capture_output=True, timeout=120)
    assert p.returncode == 0 and b"refused" not in p.stderr and p.stdout == b"".join(pile_lines(chain.ref, pileup_long_ref(chain.cases[0])[1]))
    p = subprocess.run([pl.S5PILEUP, "--refine"] + args + paths[:2], capture_output=True, timeout=120)
    assert p.returncode == 2                                                # --refine belongs to --whole
    p = subprocess.run([ct.S5CONTRAST, "-K", "3", "--refine"] + args + paths, capture_output=True, timeout=120)
    lines = cr.contrast_lines(chain.ref, want_rows, pileup_long_ref(fed[0])[1], pileup_long_ref(fed[1])[1])
    assert p.returncode == 0 and b"a.blow5: reads refused by the fit %d" % refused[0] in p.stderr and p.stdout == b"".join(lines) and len(lines) > 100, p.stderr
    t = ct.file_contrast(paths[1], paths[2], paths[0], batch=3, tile_rows=kw["tile_rows"], band=kw["band"], skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"], refine=True)
    assert len(t) == len(lines)
    t = pl.file_pileup(paths[1], paths[0], batch=3, whole=True, refine=True, tile_rows=kw["tile_rows"], band=kw["band"], skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"])
    assert t["events"].tolist() == cols["n_events"][cols["depth"] >= 1].tolist()
