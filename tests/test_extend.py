"""extend: whole-read banded alignment in tiles from map's anchor (docs/codecs.md §4.21).  The oracle is band_ref of extend_ref.py: §4.21
written in int64 numpy, with every tile's full D kept for the walk.  The CPU tests compile band_dev.h and dtw_dev.h's lane code for the host
and run 64 lanes in lockstep against it; the GPU tests hold s5gpu_event_queries_long_dev and s5gpu_sdtw_band_dev to it bit for bit."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from chain_common import DNA, EVENT, EXT_ROW, NO_COST64, PATH_ROW, PATH_WIDE, QUERY_SHORT, ROOT, host_build, levels_signal, record, synth_file, to_dev
from chain_common import gpu  # noqa: F401
from dtw_ref import path_ref, quant_ref, sdtw_ref
from extend_ref import MIXED_Q, QLENS, RLENS, SHAPES, band_ref, bparams, planted_read, planted_share, tracking_read

# the planted case: every seed that was tried is here, none was dropped
PLANTED_SEEDS = [1, 2, 3, 4, 5, 6, 7, 8]
# what band_ref gives on them, at both shapes alike: a share of events within 2 columns of the truth of 0.9980 (seed 5) to 1.0, the worst
# event 4 columns off (seeds 2 and 5), the start on the truth, the end 0 to 4 columns before it (a free end drops a last event cheaply)
PLANTED_SHARE, PLANTED_WORST = 0.998, 4


# ---------------------------------------------------------------------------------------------------------------- restatement

def test_restatement_known_answers():
    """band_ref on cases small enough to do by hand, and its uint64 cost with the per-tile renormalisation"""
    # one row, one column
    assert band_ref([5], [3], 0, 64, 64)["row"] == (2, 1, 1, 0, 0, 0, 0)
    # a diagonal: q equals r from column 2 on
    r = np.array([9, 9, 1, 2, 3, 4, 9], dtype=np.int16)
    w = band_ref([1, 2, 3, 4], r, 0, 64, 64)
    assert w["row"] == (0, 4, 1, 2, 5, 0, 0) and w["lo"].tolist() == [2, 3, 4, 5] and w["hi"].tolist() == [2, 3, 4, 5]
    # no query, a status that came in, an anchor out of range
    assert band_ref([], r, 0)["row"] == (NO_COST64, 0, 0, -1, -1, -1, 0)
    assert band_ref([1], r, 0, status_in=7)["row"][-1] == 7 and band_ref([1], r, 7)["row"][-1] == PATH_ROW and band_ref([1], r, -1)["row"][-1] == PATH_ROW
    # the windows: 65 rows in two tiles, every level held twice, against 300 levels with band 64 from anchor 100: a_0 = 100 - 16, tile 0 ends
    # in column 131, and the window follows the path
    rng = np.random.default_rng(5)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, 300)), -127, 127).astype(np.int16)
    w = band_ref(np.repeat(ref[100:133], 2)[:65], ref, 100, 64, 64)
    assert w["row"] == (0, 65, 2, 100, 132, 115, 0) and w["a"] == [84, 115]
    # the window never moves past amax = R - band, and R < band is one window from column 0
    assert band_ref(np.repeat(ref[230:265], 2), ref, 230, 64, 64)["a"] == [214, 236] and band_ref(ref[:40], ref[:40], 39, 64, 128)["a"] == [0]
    # the cost is a uint64: 65 600 rows of 32767 against the one level -32768, 65 tiles of 1024 rows, each renormalised
    Q = 65600
    w = band_ref(np.full(Q, 32767, dtype=np.int16), np.array([-32768], dtype=np.int16), 0, 1024, 64, walk=False)
    assert w["row"][0] == 65535 * Q > 1 << 32 and w["row"][2] == 65 and w["clamped"] == 0
    # ... and at emax = 2^20 rows the bound of §4.21 still holds in the arithmetic: a tile adds less than 2^29 to a carried value below 2^29
    assert 65535 * (1024 + 4096 + 64) < 1 << 29 and 65535 * (1 << 20) < 1 << 64


# ---------------------------------------------------------------------------------------------------------------- the header's code on the CPU

BAND_HOST = r'''
// The code of k_sdtw_band and k_sdtw_band_trace that lives in band_dev.h and dtw_dev.h, on the CPU.  A case of in.bin: T, band, Q, R, anchor,
// q[Q], r[R].  64 lanes in lockstep as the kernel steps them; the decision words go into slots of exactly the slot's size filled with ones,
// the carried row into band + 1 words with guards either side, the tiles' first columns into an array of exactly K entries.  out.bin gets
// the row (32 bytes), a[K], lo[Q], hi[Q] of each.
#define S5_BAND_HOST
#include "band_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace dtwk;
using namespace bandk;
static const uint32_t GUARD = 0x5A5A5A5Au;
static void shift_up1(const uint32_t *v, uint32_t fill, uint32_t *out) { for (int l = 63; l >= 1; l--) out[l] = v[l - 1]; out[0] = fill; }

struct Carry { uint32_t *S; uint32_t delta, wprev, pmin; bool first; };
static uint32_t carry_at(const Carry &C, uint32_t x) {
    bool in;
    const uint32_t at = carry_index(C.delta, x, C.wprev, &in);
    return carry_value(C.first ? 0u : C.S[at], in, C.pmin, C.first);
}

// a tile's steps: dirs_walk of dtw_dev.h with band_kernels.hip's Carry, the block fetch at every 64th step included
template <int G, int KB>
static void tile(std::vector<Lane<G, false> > &L, const int16_t *ref, uint32_t W, uint32_t nw, uint32_t *slot, const Carry &C, uint32_t wl) {
    const uint32_t SPW = 16 / G;
    uint32_t rcur[64], v[64], r[64], up[64], word[64], rblk[64], cblk[64];
    for (int l = 0; l < 64; l++) { rcur[l] = 0; rblk[l] = 0; cblk[l] = 0; }
    for (uint32_t w = 0; w < nw; w++) {
        for (int l = 0; l < 64; l++) word[l] = 0;
        for (uint32_t s = 0; s < SPW; s++) {
            const uint32_t t = w * SPW + s;
            if ((t & 63u) == 0)
                for (uint32_t l = 0; l < 64; l++) {
                    const uint32_t at = t + l;
                    rblk[l] = biased(at < W ? ref[at] : (int16_t)0);
                    cblk[l] = at < W ? carry_at(C, at + 1u) : FAR;
                }
            shift_up1(rcur, rblk[t & 63u], r);
            for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
            shift_up1(v, cblk[t & 63u], up);
            for (uint32_t l = 0; l < 64; l++) {
                const uint32_t j = t - l;
                word[l] = path_pack(word[l], lane_step_dirs(L[l], r[l], up[l]), s, G);
                lane_best<G, false, KB>(L[l], j, W);
                if (l == wl && j < W) C.S[j + 1u] = L[l].d[KB];
            }
        }
        for (int l = 0; l < 64; l++) slot[(size_t)w * 64 + l] = word[l];
    }
}
template <int G, int KB = 0>
struct Pick {
    static void go(int kb, std::vector<Lane<G, false> > &L, const int16_t *ref, uint32_t W, uint32_t nw, uint32_t *slot, const Carry &C, uint32_t wl) {
        if (kb == KB) return tile<G, KB>(L, ref, W, nw, slot, C, wl);
        if constexpr (KB + 1 < G) return Pick<G, KB + 1>::go(kb, L, ref, W, nw, slot, C, wl);
        abort();
    }
};

template <int G>
static int band(uint32_t bandw, const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R, int32_t anchor, FILE *o) {
    const uint32_t T = 64u * G, K = tiles_of(Q, T), slot_words = path_slot_words(T, bandw);
    std::vector<int32_t> lo(Q, -1), hi(Q, -1);
    s5gpu_ext_row_t row = row_none(S5GPU_STATUS_PATH_ROW);
    if (anchor < 0 || (uint32_t)anchor >= R) {
        fwrite(&row, sizeof row, 1, o);
        fwrite(lo.data(), 4, Q, o); fwrite(hi.data(), 4, Q, o);
        return 0;
    }
    uint32_t *slots = (uint32_t *)malloc((size_t)K * slot_words * 256);
    int32_t *tile_a = (int32_t *)malloc((size_t)K * 4);
    uint32_t *carry = (uint32_t *)malloc(((size_t)bandw + 3) * 4);
    if (!slots || !tile_a || !carry) return -1;
    memset(slots, 0xFF, (size_t)K * slot_words * 256);
    for (uint32_t x = 0; x < bandw + 3; x++) carry[x] = GUARD;
    Carry C;
    C.S = carry + 1; C.delta = 0; C.wprev = 0; C.pmin = 0; C.first = true;
    C.S[0] = FAR;
    const uint32_t amax = win_amax(R, bandw);
    uint32_t a = win_place((uint32_t)anchor, bandw, 0u, amax), end = 0;
    uint64_t base = 0;
    bool bad = false;
    for (uint32_t k = 0; k < K && !bad; k++) {
        const uint32_t Qk = tile_rows_of(Q, T, k), W = win_cols(a, R, bandw), last = (Qk - 1u) / G;
        const int kb = (int)(Qk - 1u - last * G);
        std::vector<Lane<G, false> > L(64);
        for (uint32_t l = 0; l < 64; l++) {
            lane_init(L[l], false);
            for (int kk = 0; kk < G; kk++) { const uint32_t r = k * T + l * G + kk; L[l].q[kk] = biased(r < Q ? q[r] : (int16_t)0); }
        }
        L[0].dg = carry_at(C, 0u);
        uint32_t nw = path_words(G, W + last);
        if (nw > slot_words) abort();
        tile_a[k] = (int32_t)a;
        Pick<G>::go(kb, L, ref + a, W, nw, slots + (size_t)k * slot_words * 64, C, k + 1u < K ? 63u : 64u);
        const uint32_t mn = L[last].best, m = (uint32_t)L[last].best_end;
        if (m >= W || mn >= FAR) { bad = true; break; }
        base += mn;
        end = a + m;
        const uint32_t an = win_place(end, bandw, a, amax);
        C.delta = an - a; C.wprev = W; C.pmin = mn; C.first = false;
        if (k + 1u < K) a = an;
    }
    if (carry[0] != GUARD || carry[bandw + 2] != GUARD) abort();
    if (!bad) {
        int32_t start = -1;
        const int32_t rc = band_walk(slots, slot_words, tile_a, G, T, bandw, Q, R, (int32_t)end, lo.data(), hi.data(), &start);
        if (rc == 0) { row.cost = base; row.qlen = Q; row.tiles = K; row.start = start; row.end = (int32_t)end; row.a_last = (int32_t)a; row.status = 0; }
        else for (uint32_t i = 0; i < Q; i++) { lo[i] = -1; hi[i] = -1; }
    }
    fwrite(&row, sizeof row, 1, o);
    if (row.status == 0) fwrite(tile_a, 4, K, o);
    fwrite(lo.data(), 4, Q, o); fwrite(hi.data(), 4, Q, o);
    free(slots); free(tile_a); free(carry);
    return 0;
}

static int one_case(FILE *f, FILE *o) {
    uint32_t h[4];
    int32_t anchor;
    if (fread(h, 4, 4, f) != 4) return 1;
    const uint32_t T = h[0], bandw = h[1], Q = h[2], R = h[3];
    if (fread(&anchor, 4, 1, f) != 1 || !tile_ok(T) || !band_ok(bandw) || Q < 1 || Q > EMAX || R < 1) return -1;
    std::vector<int16_t> q(Q), r(R);
    if (fread(q.data(), 2, Q, f) != Q || fread(r.data(), 2, R, f) != R) return -1;
    switch (T) {
    case 64: return band<1>(bandw, q.data(), Q, r.data(), R, anchor, o);
    case 128: return band<2>(bandw, q.data(), Q, r.data(), R, anchor, o);
    case 256: return band<4>(bandw, q.data(), Q, r.data(), R, anchor, o);
    case 512: return band<8>(bandw, q.data(), Q, r.data(), R, anchor, o);
    case 1024: return band<16>(bandw, q.data(), Q, r.data(), R, anchor, o);
    }
    return -1;
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 1;
    for (;;) {
        const int rc = one_case(f, o);
        if (rc < 0) return 1;
        if (rc > 0) break;
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def host_cases():
    """-> [(T, band, q, r, anchor)]: every shape of SHAPES with every Q of QLENS against every R of RLENS (tracking reads, anchors at 0, at
    R - 1 and a few columns off the read's start), tie-dense {-1, 0, 1} values, the extremes 32767 against -32768 over four tiles, an anchor
    out of range, and the larger tiles once each"""
    rng = np.random.default_rng(61)
    cases = []
    for T, band in SHAPES:
        for Q in QLENS:
            for n, R in enumerate(RLENS):
                q, r, anchor = tracking_read(rng, Q, R)
                anchor = (anchor, 0, R - 1)[(n + Q) % 3]
                cases.append((T, band, q, r, anchor))
        for Q, R in ((129, 65), (200, 300), (321, 40)):
            cases.append((T, band, rng.integers(-1, 2, Q).astype(np.int16), rng.integers(-1, 2, R).astype(np.int16), int(rng.integers(0, R))))
        Q, R = 3 * T + 7, 300
        r = np.full(R, -32768, dtype=np.int16)
        cases.append((T, band, np.full(Q, 32767, dtype=np.int16), r, 150))
        r = r.copy()
        r[rng.integers(0, R, 40)] = 32767
        cases.append((T, band, np.where(rng.integers(0, 4, Q) == 0, -32768, 32767).astype(np.int16), r, 20))
        cases.append((T, band, np.zeros(5, dtype=np.int16), np.zeros(9, dtype=np.int16), 9))      # the anchor is out of range
    for T, band, Q, R in ((256, 512, 700, 900), (256, 256, 300, 1000), (512, 64, 1100, 200), (1024, 128, 1030, 400), (64, 4096, 130, 4500)):
        q, r, anchor = tracking_read(rng, Q, R)
        cases.append((T, band, q, r, anchor))
    return cases


def _build_band_host(tmp_path, extra=()):
    return host_build(tmp_path, "band_host", BAND_HOST, ["-O1", "-std=c++17", "-ffp-contract=off"], extra)


def write_host_cases(path, cases):
    with open(path, "wb") as fh:
        for T, band, q, r, anchor in cases:
            fh.write(struct.pack("<IIIIi", T, band, len(q), len(r), anchor) + np.asarray(q, dtype=np.int16).tobytes() + np.asarray(r, dtype=np.int16).tobytes())


def _same_result(what, want, row, a, lo, hi):
    assert tuple(row.tolist()) == want["row"], (what, row, want["row"])
    if want["row"][-1] == 0 and want["row"][1]:
        assert a is None or list(a) == want["a"], (what, a, want["a"])
        assert np.array_equal(lo, want["lo"]) and np.array_equal(hi, want["hi"]), what
    else:
        assert (np.asarray(lo) == -1).all() and (np.asarray(hi) == -1).all(), what


def test_the_band_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """carry_index, carry_value, win_place, band_walk of band_dev.h and lane_step_dirs, lane_best of dtw_dev.h as g++ compiles them, on
    host_cases(): rows, every a_k, lo and hi equal band_ref's"""
    cases = host_cases()
    exe = _build_band_host(tmp_path)
    write_host_cases(tmp_path / "in.bin", cases)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw, at = (tmp_path / "out.bin").read_bytes(), 0
    moved, stuck, tiles = 0, 0, set()
    for T, band, q, r, anchor in cases:
        Q = len(q)
        want = band_ref(q, r, anchor, T, band)
        row = np.frombuffer(raw, EXT_ROW, 1, at)[0]
        at += 32
        a = None
        if row["status"] == 0:
            a = np.frombuffer(raw, np.int32, int(row["tiles"]), at).tolist()
            at += 4 * int(row["tiles"])
        lo, hi = np.frombuffer(raw, np.int32, Q, at), np.frombuffer(raw, np.int32, Q, at + 4 * Q)
        at += 8 * Q
        _same_result((T, band, Q, len(r), anchor), want, row, a, lo, hi)
        assert want["clamped"] == 0
        if a:
            tiles.add(len(a))
            moved += len(set(a)) > 1
            stuck += len(a) > 1 and a[-1] == max(len(r) - band, 0)
    assert at == len(raw)
    assert {1, 2, 3, 4, 6} <= tiles and moved >= 10 and stuck >= 10


def test_a_band_as_wide_as_the_reference_is_the_full_matrix():
    """band >= R: every window is the whole reference, and cost, lo and hi are §4.16's and §4.17's of the full matrix (path_ref), whatever the
    tiling: random and tie-dense cases, Q <= 400"""
    rng = np.random.default_rng(17)
    n = 0
    for T, band in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256)):
        for kind in range(9):
            Q = int(rng.integers(1, 401))
            R = int(rng.integers(1, band + 1))
            if kind % 3 == 0:
                q, r = rng.integers(-1, 2, Q).astype(np.int16), rng.integers(-1, 2, R).astype(np.int16)
            elif kind % 3 == 1:
                q, r = rng.integers(-127, 128, Q).astype(np.int16), rng.integers(-127, 128, R).astype(np.int16)
            else:
                q, r, _ = tracking_read(rng, Q, R)
            cost, lo, hi = path_ref(q, r, cross_check=Q <= 200)
            w = band_ref(q, r, int(rng.integers(0, R)), T, band)
            assert w["row"] == (cost, Q, (Q + T - 1) // T, int(lo[0]), int(hi[-1]), 0, 0), (T, band, Q, R)
            assert np.array_equal(w["lo"], lo) and np.array_equal(w["hi"], hi), (T, band, Q, R)
            n += 1
    assert n >= 40


@pytest.mark.parametrize("T,band", [(64, 128), (256, 512)])
def test_the_planted_case(T, band):
    """§4.21's planted case in the restatement, on every seed of PLANTED_SEEDS: the share of events within 2 columns of the truth is at least
    PLANTED_SHARE, and no event, the two ends included, is more than PLANTED_WORST columns off"""
    for seed in PLANTED_SEEDS:
        q, ref, anchor, truth = planted_read(seed)
        w = band_ref(q, ref, anchor, T, band)
        share, worst = planted_share(w, truth)
        print("planted seed %d (%d, %d): share %.4f worst %d cost/event %.2f" % (seed, T, band, share, worst, w["row"][0] / len(q)))
        assert share >= PLANTED_SHARE and worst <= PLANTED_WORST, (seed, share, worst)
        assert abs(w["row"][3] - truth[0]) <= PLANTED_WORST and abs(w["row"][4] - truth[-1]) <= PLANTED_WORST, (seed, w["row"], truth[0], truth[-1])
        assert w["clamped"] == 0


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3): the pointers are never dereferenced on the host, so made-up aligned addresses serve"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    A = 1 << 20
    nan, inf = float("nan"), float("inf")
    bad_params = [dict(emin=0), dict(emin=11, emax=10), dict(emax=(1 << 20) + 1), dict(emax=0), dict(tile_rows=0), dict(tile_rows=32), dict(tile_rows=192),
                  dict(tile_rows=2048), dict(band=0), dict(band=32), dict(band=96), dict(band=4160), dict(band=1 << 31), dict(clip=0), dict(clip=32768),
                  dict(clip=-1), dict(scale=0.0), dict(scale=-1.0), dict(scale=nan), dict(scale=inf)]

    def ql(n=4, rows=A, first=A, es=A, P=None, pnull=False, total=100, q=A, qlen=A, st=A):
        p = P or bparams()
        return L.s5gpu_event_queries_long_dev(n, rows, first, es, None if pnull else C.byref(p), total, q, qlen, st, None)
    assert ql(pnull=True) == -1
    for kw in bad_params:
        assert ql(P=bparams(**kw)) == -1, kw
    for name in ("rows", "first", "q", "qlen", "st"):
        assert ql(**{name: None}) == -1, name
    assert ql(rows=A + 8) == -1 and ql(first=A + 4) == -1 and ql(es=A + 2) == -1 and ql(q=A + 1) == -1 and ql(qlen=A + 2) == -1 and ql(st=A + 2) == -1
    assert ql(n=0) == 0 and ql(n=0, first=None, q=None) == 0               # nothing to do: nothing is launched

    sb = L.s5gpu_sdtw_band_scratch_bytes
    assert sb(4, 100, 32, 512) == 0 and sb(4, 100, 256, 96) == 0 and sb(4, 100, 256, 8192) == 0
    slot = L.s5gpu_sdtw_path_slot_bytes(256, 512)
    assert slot == 144 * 256 and sb(1, 20000, 256, 512) == 79 * slot + 320 and sb(4, 1000, 256, 512) == 7 * slot + 32 and sb(0, 0, 64, 64) == 0
    assert sb(3, 129, 64, 128) == 5 * L.s5gpu_sdtw_path_slot_bytes(64, 128) + 32

    def bd(n=4, q=A, first=A, qlen=A, total=1000, ref=A, R=100, an=A, si=A, P=None, pnull=False, scratch=A, sbytes=1 << 30, ro=A, lo=A, hi=A):
        p = P or bparams()
        return L.s5gpu_sdtw_band_dev(n, q, first, qlen, total, ref, R, an, si, None if pnull else C.byref(p), scratch, sbytes, ro, lo, hi, None)
    assert bd(pnull=True) == -1 and bd(R=0) == -1 and bd(R=1 << 31) == -1 and bd(ref=None) == -1 and bd(total=(1 << 40) + 1) == -1
    for kw in bad_params:
        assert bd(P=bparams(**kw)) == -1, kw
    for name in ("q", "first", "qlen", "an", "si", "scratch", "ro", "lo", "hi"):
        assert bd(**{name: None}) == -1, name
    assert bd(q=A + 1) == -1 and bd(first=A + 4) == -1 and bd(qlen=A + 2) == -1 and bd(ref=A + 1) == -1 and bd(an=A + 2) == -1 and bd(si=A + 1) == -1
    assert bd(scratch=A + 8) == -1 and bd(ro=A + 8) == -1 and bd(lo=A + 2) == -1 and bd(hi=A + 1) == -1
    need = sb(4, 1000, 256, 512)
    assert bd(sbytes=need - 1) == -3 and bd(sbytes=need - slot) == -3 and bd(sbytes=0) == -3
    assert bd(n=0) == 0 and bd(n=0, sbytes=0, q=None, ro=None) == 0
    # the batch call: the cases of s5gpu_map_batch, the band parameters, the outputs
    vp = C.c_void_p
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    h_map, h_rows, h_first = np.full(16, 0xA5, dtype=np.uint8), np.full(32, 0xA5, dtype=np.uint8), np.full(2, 77, dtype=np.uint64)
    h_lo, h_hi, h_st = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)

    def batch(pr=(0, 64, 10, 32.0, 127, 1), ev=DNA, P=None, pnull=False, R=100, ref=True, mrows=True, rows=True, first=True, lo=True, methods=(1, 1)):
        e, p, bp = _lib.EventParams(*ev), _lib.MapParams(*pr), P or bparams(emin=10)
        return L.s5gpu_extend_batch(1, rec_p, rl, methods[0], methods[1], C.byref(e), C.byref(p), None if pnull else C.byref(bp), 0,
                                    h_ref.ctypes.data_as(vp) if ref else None, R, h_map.ctypes.data_as(vp) if mrows else None,
                                    h_rows.ctypes.data_as(vp) if rows else None, h_first.ctypes.data_as(vp) if first else None,
                                    h_lo.ctypes.data_as(vp) if lo else None, h_hi.ctypes.data_as(vp), None, 64, h_st.ctypes.data_as(vp))
    for pr in ((0, 0, 1, 32.0, 127, 1), (0, 1025, 1, 32.0, 127, 1), (0, 64, 0, 32.0, 127, 1), (0, 64, 10, nan, 127, 1), (0, 64, 10, 32.0, 0, 1)):
        assert batch(pr=pr) == -1, pr
    assert batch(R=0) == -1 and batch(ref=False) == -1 and batch(pnull=True) == -1 and batch(methods=(9, 1)) == -1
    assert batch(mrows=False) == -1 and batch(rows=False) == -1 and batch(first=False) == -1 and batch(lo=False) == -1
    for kw in bad_params:
        assert batch(P=bparams(**dict(dict(emin=10), **kw))) == -1, kw
    assert batch(P=bparams(emin=10, skip=1)) == -1 and batch(P=bparams(emin=10, clip=100)) == -1 and batch(P=bparams(emin=10, scale=16.0)) == -1
    assert (h_map == 0xA5).all() and (h_rows == 0xA5).all() and (h_first == 77).all() and (h_lo == -7).all() and (h_hi == -7).all() and (h_st == -7).all()


def test_library_exports_the_extend_calls():
    """the symbols are in the header, in the library and in the bindings' list"""
    from slow5tools_amd import _lib, extend

    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "slow5gpu.h")).read()
    for name in ("s5gpu_event_queries_long_dev", "s5gpu_sdtw_band_scratch_bytes", "s5gpu_sdtw_band_dev", "s5gpu_extend_batch"):
        assert hasattr(L, name) and name in _lib.EXPORTS and name + "(" in hdr, name
    assert os.access(extend.S5EXTEND, os.X_OK)
    for bad in (0, 4, -1):
        assert L.s5gpu_set_option(b"sdtw_band_passes", bad) == -1
    assert L.s5gpu_set_option(b"sdtw_band_passes", 1) == 0 and L.s5gpu_set_option(b"sdtw_band_passes", 3) == 0
    assert subprocess.run([extend.S5EXTEND], capture_output=True).returncode == 2
    assert extend.EXT_ROW == EXT_ROW and C.sizeof(_lib.BandParams) == 32
    p = extend.BandParams()
    assert (p.tile_rows, p.band, p.emax) == (256, 512, 1 << 20)


# ---------------------------------------------------------------------------------------------------------------- gpu

class Reads:
    """event rows of n reads, ragged, whose means follow a reference from an anchor; what quant_ref makes of them is the host's query"""

    def __init__(self, R, qlens, skip, seed, failed=()):
        rng = np.random.default_rng(seed)
        self.skip, self.R = skip, R
        self.ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
        means, self.first, self.anchor, self.q, self.ev_status = [], [0], [], [], []
        for i, Q in enumerate(qlens):
            E = 0 if Q == 0 and i % 2 else Q + skip if Q else max(skip - 1, 0)      # a read without a query: no rows, or too few
            s = int(rng.integers(0, R))
            cols = np.minimum(s + np.cumsum(rng.integers(0, 2, E)), R - 1)
            if i % 5 == 4:
                m = rng.integers(-1, 2, E).astype(np.float32)              # tie-dense
            else:
                m = (self.ref[cols] * 3.0 + 500.0 + rng.normal(0.0, 4.0, E)).astype(np.float32)
            means.append(m)
            self.first.append(self.first[-1] + E)
            self.anchor.append((int(np.clip(s + rng.integers(-5, 6), 0, R - 1)), 0, R - 1)[i % 3])
            self.ev_status.append(7 if i in failed else 0)
            self.q.append(quant_ref(m[skip:skip + Q]) if Q and i not in failed else np.zeros(0, dtype=np.int16))
        self.n, self.total = len(qlens), self.first[-1]
        self.rows = np.zeros(self.total, dtype=EVENT)
        self.rows["mean"] = np.concatenate(means) if means else np.zeros(0, dtype=np.float32)
        self.rows["length"] = 5

    def want_status(self, i, emin):
        return self.ev_status[i] if self.ev_status[i] else QUERY_SHORT if len(self.q[i]) < emin else 0


def _run_band(env, rd, T, band, emin=1, anchor=None, scratch_bytes_=None):
    ex, t = env.extend, env.torch
    p = ex.BandParams(rd.skip, emin, 1 << 20, T, band)
    d_rows, d_first = to_dev(env, rd.rows.view(np.int32).reshape(-1, 4)), to_dev(env, np.array(rd.first, dtype=np.int64))
    q, ql, st = ex.queries_long_dev(d_rows, d_first, to_dev(env, np.array(rd.ev_status, dtype=np.int32)), p)
    rows, lo, hi = ex.band_dev(q, d_first, ql, to_dev(env, rd.ref), to_dev(env, np.array(rd.anchor if anchor is None else anchor, dtype=np.int32)), st, p, scratch_bytes_)
    t.cuda.synchronize()
    return q.cpu().numpy(), ql.cpu().numpy(), st.cpu().numpy(), rows.cpu().numpy().view(EXT_ROW).reshape(-1), lo.cpu().numpy(), hi.cpu().numpy()


def _check_band(rd, got, T, band, emin=1, anchor=None, wants=None):
    q, ql, st, rows, lo, hi = got
    wants = {} if wants is None else wants
    for i in range(rd.n):
        f0, f1 = rd.first[i], rd.first[i + 1]
        ws = rd.want_status(i, emin)
        wq = rd.q[i] if ws == 0 else np.zeros(0, dtype=np.int16)
        Q = len(wq)
        assert ql[i] == Q and st[i] == ws, (i, ql[i], st[i], ws)
        assert np.array_equal(q[f0:f0 + Q], wq) and not q[f0 + Q:f1].any(), i
        an = (rd.anchor if anchor is None else anchor)[i]
        key = (i, T, band, an)
        if key not in wants:
            wants[key] = band_ref(wq, rd.ref, an, T, band, status_in=ws)
        _same_result((i, Q, T, band), wants[key], rows[i], None, lo[f0:f0 + Q], hi[f0:f0 + Q])
        assert (lo[f0 + Q:f1] == -1).all() and (hi[f0 + Q:f1] == -1).all(), i
    return wants


@pytest.mark.gpu
@pytest.mark.parametrize("R", [65, 300])
@pytest.mark.parametrize("T,band", SHAPES)
def test_band_is_exact_on_a_mixed_batch(gpu, R, T, band):
    """40 reads through queries_long_dev and band_dev: every Q of QLENS, reads without rows or with fewer than skip + 1, and a failed one,
    anchors at 0, at R - 1 and near the read; rows, lo and hi equal band_ref's of quant_ref's query"""
    rd = Reads(R, MIXED_Q, skip=3, seed=900 + R, failed=(7,))
    got = _run_band(gpu, rd, T, band)
    _check_band(rd, got, T, band)
    st = got[2]
    assert st[7] == 7 and st[36] == QUERY_SHORT and st[37] == QUERY_SHORT and (st == 0).sum() == 37
    assert got[3]["status"][7] == 7 and got[3]["cost"][7] == NO_COST64 and got[3]["status"][36] == QUERY_SHORT


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_band_every_row_of_the_last_lane(gpu, G):
    """tiles of T = 64 G rows: reads of T - k rows, k < G (one tile, no row carried out), and of 2 T - k (two tiles), so that the last row of
    the last tile is every row (Qk - 1) % G of the lane that holds it: the walks are compiled per such row"""
    T, band = 64 * G, 64
    qs = [T - k for k in range(G)] + [2 * T - k for k in range(G)]
    assert {(Q - 1) % G for Q in qs[:G]} == set(range(G)) and {(Q - T - 1) % G for Q in qs[G:]} == set(range(G))
    rd = Reads(300, qs, skip=3, seed=950 + G)
    wants = {(i, T, band, rd.anchor[i]): band_ref(rd.q[i], rd.ref, rd.anchor[i], T, band) for i in range(rd.n)}
    assert [w["row"][1:3] for w in wants.values()] == [(Q, 1 + (i >= G)) for i, Q in enumerate(qs)]
    assert all(w["row"][6] == 0 and w["row"][0] < NO_COST64 and w["lo"][0] >= 0 for w in wants.values())       # every read has a result
    _check_band(rd, _run_band(gpu, rd, T, band), T, band, wants=wants)


@pytest.mark.gpu
@pytest.mark.parametrize("T,band,R", [(256, 512, 900), (512, 64, 200), (1024, 128, 400), (64, 4096, 4500)])
def test_band_is_exact_with_the_larger_tiles_and_bands(gpu, T, band, R):
    """the default shape with Q up to 700, the two largest tiles, and the widest band (its LDS is above 64 KiB a workgroup)"""
    qs = {256: [700, 513, 256, 257, 1, 300], 512: [1100, 512, 513, 40], 1024: [1030, 1024, 2049, 77], 64: [130, 64, 200]}[T]
    rd = Reads(R, qs, skip=0, seed=77 + T)
    _check_band(rd, _run_band(gpu, rd, T, band), T, band)


@pytest.mark.gpu
def test_band_over_many_workgroups_and_an_anchor_out_of_range(gpu):
    """300 reads, 75 workgroups: the slots of read i start at floor(first[i] / T) + i, whatever workgroup it is in; emin 64 leaves the reads of
    1 and 63 rows without a query; and anchors out of range"""
    base = Reads(300, [QLENS[i % len(QLENS)] for i in range(300)], skip=1, seed=31)
    got = _run_band(gpu, base, 64, 128)
    wants = _check_band(base, got, 64, 128)
    got = _run_band(gpu, base, 64, 128, emin=64)
    _check_band(base, got, 64, 128, emin=64, wants={k: v for k, v in wants.items() if len(base.q[k[0]]) >= 64})
    assert (got[2] == QUERY_SHORT).sum() == 68 and (got[3]["status"] == QUERY_SHORT).sum() == 68
    anchor = list(base.anchor)
    anchor[0], anchor[5], anchor[299] = -1, 300, 1 << 30
    got = _run_band(gpu, base, 64, 128, anchor=anchor)
    _check_band(base, got, 64, 128, anchor=anchor)
    assert got[3]["status"][[0, 5, 299]].tolist() == [PATH_ROW] * 3 and not got[3]["status"][1:5].any()


@pytest.mark.gpu
def test_a_scratch_one_slot_too_small_is_refused_and_nothing_is_written(gpu):
    ex, t = gpu.extend, gpu.torch
    rd = Reads(300, [200, 129, 64], skip=0, seed=3)
    p = ex.BandParams(0, 1, 1 << 20, 64, 128)
    d_rows, d_first = to_dev(gpu, rd.rows.view(np.int32).reshape(-1, 4)), to_dev(gpu, np.array(rd.first, dtype=np.int64))
    q, ql, st = ex.queries_long_dev(d_rows, d_first, None, p)
    need = ex.scratch_bytes(rd.n, rd.total, 64, 128)
    slot = gpu.L.s5gpu_sdtw_path_slot_bytes(64, 128)
    slots = rd.total // 64 + rd.n
    assert need == slots * slot + (4 * slots + 15) // 16 * 16
    rows = t.full((rd.n, 4), -3, dtype=t.int64, device="cuda")
    lo, hi = t.full((rd.total,), -3, dtype=t.int32, device="cuda"), t.full((rd.total,), -3, dtype=t.int32, device="cuda")
    scratch = t.full((need // 4,), -3, dtype=t.int32, device="cuda")
    ref, an, zero = to_dev(gpu, rd.ref), to_dev(gpu, np.array(rd.anchor, dtype=np.int32)), t.zeros(rd.n, dtype=t.int32, device="cuda")
    rc = gpu.L.s5gpu_sdtw_band_dev(rd.n, q.data_ptr(), d_first.data_ptr(), ql.data_ptr(), rd.total, ref.data_ptr(), rd.R, an.data_ptr(), zero.data_ptr(),
                                   C.byref(p), scratch.data_ptr(), need - slot, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(), None)
    t.cuda.synchronize()
    assert rc == -3 and b"scratch" in gpu.L.s5gpu_last_error()
    assert (rows == -3).all() and (lo == -3).all() and (hi == -3).all() and (scratch == -3).all()
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-3"):
        ex.band_dev(q, d_first, ql, ref, an, None, p, scratch_bytes_=need - 1)


@pytest.mark.gpu
def test_extend_end_to_end_on_a_synthetic_file(gpu, tmp_path):
    """extend_dev, read_extend (s5gpu_extend_batch, in two groups) and file_extend (s5extend) equal the chain restated on the host: the events
    of the library's own event call, quant_ref, the anchor from sdtw_ref on the prefix, band_ref.  Reads of about 2000 events, one read too
    short, one record corrupt; the reference holds the levels of reads 0 and 4"""
    ex = gpu.extend
    rng = np.random.default_rng(47)
    lengths = [24000, 20000, 40, 5000, 22000]
    recs = [record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
    bad = bytearray(recs[3])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[3] = bytes(bad)
    n, skip, qmax, qmin, T, band = len(recs), 2, 100, 20, 64, 128
    ids = [ob.synth_read_id(i) for i in range(n)]
    ids = [i if isinstance(i, bytes) else i.encode() for i in ids]
    dec = gpu.press.decode_to_device(recs)
    ev_rows, first = gpu.events.events_dev(dec, DNA, "raw")
    h_ev, h_first = ev_rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    E = np.diff(h_first)
    assert E[0] > 1500 and E[1] > 1200 and E[4] > 1400 and E[2] < qmin and E[3] == 0
    m0, m4 = h_ev["mean"][h_first[0]:h_first[1]], h_ev["mean"][h_first[4]:h_first[5]]
    levels = np.concatenate([rng.normal(500.0, 110.0, 300), m0, rng.normal(500.0, 110.0, 200), m4, rng.normal(500.0, 110.0, 100)]).astype(np.float32)
    ref = quant_ref(levels)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n" + "".join("%.9g\n" % v for v in levels))
    kw = dict(skip=skip, qmax=qmax, qmin=qmin, tile_rows=T, band=band)
    # the chain restated on the host
    want, anchors = {}, {}
    for i in (0, 1, 4):
        m = h_ev["mean"][h_first[i] + skip:h_first[i + 1]]
        anchors[i] = sdtw_ref(quant_ref(m[:qmax]), ref)
        want[i] = band_ref(quant_ref(m), ref, anchors[i][1], T, band)
    cpe = {i: want[i]["row"][0] / want[i]["row"][1] for i in want}
    print("cost per event", cpe, "starts", [want[i]["row"][3] for i in want])
    assert abs(want[0]["row"][3] - (300 + skip)) <= 4 and abs(want[0]["row"][4] - (300 + E[0] - 1)) <= 4               # a read on its own levels
    assert 2 * cpe[0] < cpe[1] and 2 * cpe[4] < cpe[1]                                                                 # ... and one on none

    def same(i, row, lo, hi):
        assert tuple(row.tolist()) == want[i]["row"], (i, row, want[i]["row"])
        assert np.array_equal(lo, want[i]["lo"]) and np.array_equal(hi, want[i]["hi"]), i
    # the device chain of extend_dev
    mrows, X = ex.extend_dev(dec, ref, **kw)
    for i in (0, 1, 4):
        Q = int(X.rows[i]["qlen"])
        assert mrows[i].tolist() == (anchors[i][0], qmax, anchors[i][1], anchors[i][2]) and Q == E[i] - skip
        same(i, X.rows[i], X.lo[h_first[i]:h_first[i] + Q], X.hi[h_first[i]:h_first[i] + Q])
    assert X.rows[2].tolist() == (NO_COST64, 0, 0, -1, -1, -1, QUERY_SHORT) and X.rows[3]["qlen"] == 0 and X.rows[3]["status"] not in (0, QUERY_SHORT)
    # the batch call, in two groups: reads 0 and 1, then the rest
    two = ex.scratch_bytes(2, int(E[0] + E[1]), T, band)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        ex.read_extend(recs, ref, **kw)
    for smax in (0, two):
        b_map, b_rows, b_first, b_lo, b_hi, b_ev, b_st = ex.read_extend(recs, ref, raise_on_error=False, scratch_max=smax, **kw)
        assert b_map.tolist() == mrows.tolist() and b_first.tolist() == np.concatenate([[0], np.cumsum(b_rows["qlen"])]).tolist()
        for i in (0, 1, 4):
            f0, f1 = int(b_first[i]), int(b_first[i + 1])
            same(i, b_rows[i], b_lo[f0:f1], b_hi[f0:f1])
            assert b_ev[f0:f1].tobytes() == h_ev[h_first[i] + skip:h_first[i + 1]].tobytes() and b_st[i] == 0
        assert b_rows[2].tolist() == (NO_COST64, 0, 0, -1, -1, -1, QUERY_SHORT) and b_st[2] == QUERY_SHORT
        assert b_rows[3]["qlen"] == 0 and b_rows[3]["status"] == b_st[3] and b_st[3] not in (0, QUERY_SHORT, PATH_ROW, PATH_WIDE)
    # a read whose scratch alone is above scratch_max has no path; the others stay valid
    one = ex.scratch_bytes(1, int(E[1]), T, band)
    b_map, b_rows, b_first, b_lo, b_hi, b_ev, b_st = ex.read_extend(recs, ref, raise_on_error=False, scratch_max=one, **kw)
    assert b_st.tolist()[:3] == [PATH_WIDE, 0, QUERY_SHORT] and b_st[4] == PATH_WIDE and b_rows[0].tolist() == (NO_COST64, 0, 0, -1, -1, -1, PATH_WIDE)
    same(1, b_rows[1], b_lo, b_hi)
    assert b_first.tolist() == [0, 0, E[1] - skip, E[1] - skip, E[1] - skip, E[1] - skip]
    # the tool: exit 1, the corrupt read named, the other reads' lines
    synth_file(tmp_path / "reads.blow5", recs)
    args = ["--skip", str(skip), "--events", str(qmax), "--min-events", str(qmin), "--tile", str(T), "--band", str(band), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([ex.S5EXTEND, "-K", "2"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[3] in p.stderr and b"short" in p.stderr, p.stderr
    keep = [0, 1, 2, 4]
    lines = []
    for i in keep:
        if i == 2:
            lines.append(ids[i] + b"\t*" * 7 + b"\n")
            continue
        c, Q, K, s0, e0 = want[i]["row"][:5]
        lines.append(b"%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (ids[i], Q, c, b"%.3f" % (c / Q), s0, e0, K, anchors[i][1]))
    assert p.stdout == b"".join(lines)
    fids, flines = ex.file_extend(tmp_path / "reads.blow5", ref_txt, batch=2, raise_on_corrupt=False, **kw)
    assert fids == [ids[i] for i in keep] and flines["cost"].tolist() == [want[i]["row"][0] if i in want else -1 for i in keep]
    assert flines["anchor"].tolist() == [anchors[i][1] if i in anchors else -1 for i in keep]
    with pytest.raises(gpu.lib.S5GpuError):
        ex.file_extend(tmp_path / "reads.blow5", ref_txt, **kw)
    # --per-event: s5align's lines for every event of the whole read
    p = subprocess.run([ex.S5EXTEND, "--per-event"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1
    lines = []
    for i in keep:
        if i == 2:
            lines.append(ids[i] + b"\t*\t*\t*\t*\t*\t*\n")
            continue
        for k in range(len(want[i]["lo"])):
            e = h_ev[h_first[i] + skip + k]
            lines.append(b"%s\t%d\t%d\t%d\t%s\t%d\t%d\n" % (ids[i], skip + k, e["start"], e["start"] + e["length"], b"%.6g" % float(e["mean"]), want[i]["lo"][k],
                                                            want[i]["hi"][k]))
    assert p.stdout == b"".join(lines)
    # --max-events reaches the call; bad options are refused
    p = subprocess.run([ex.S5EXTEND, "--max-events", "500"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and [l.split(b"\t")[1] for l in p.stdout.splitlines()] == [b"500", b"500", b"*", b"500"]
    for badarg in (["--tile", "96"], ["--band", "100"], ["--max-events", "10"]):
        assert subprocess.run([ex.S5EXTEND] + args[:-2] + badarg + args[-2:], capture_output=True).returncode == 2, badarg
