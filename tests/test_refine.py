"""refine: per-read level rescaling from the path, and a windowed realign, on the device (docs/codecs.md §4.20;
slow5tools_amd/csrc/refine_kernels.hip).

The oracle is in refine_ref.py: the fit in Python integers and np.float64 in the order §4.20 states (fit_ref), the requantiser (requant_ref),
and the realign as dtw_ref.path_ref, the FULL matrix of §4.16 / §4.17, on the slice of the reference that is the window (window_ref);
refine_ref iterates them.  Sums, a, b, q', rows, lo, hi, statuses and rounds are held to it exactly.  refine_dev.h and the new walk of dtw_dev.h are
plain C++: they are also compiled for the CPU, 64 lanes in lockstep over the window, and held to the same oracle.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from chain_common import DNA, EMPTY, EVENT, FIT, FIT_FLAT, FIT_RANGE, GUARD, MAP_ROW, PATH_ROW, PATH_WIDE, QUERY_SHORT, ROOT
from chain_common import host_build, levels_signal, record, synth_file, to_dev
from chain_common import gpu  # noqa: F401
from dtw_ref import _g_of, last_lane_batch, path_ref, quant_ref
from refine_ref import FIT_NONE, c_params, fit_ref, params, params_bytes, path_status_ref, planted, planted_refined, refine_ref, requant_ref, round_ref, window_ref

QLENS = [1, 63, 64, 65, 128, 129, 256, 257, 513, 1024]                     # every lane height and its seams
PADS = [0, 1, 64]
PLANTED_SEED = 276                                                         # the conditions of test_the_planted_case hold for it

# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = ["s5gpu_path_fit_dev", "s5gpu_sdtw_window_dev", "s5gpu_refine_work_bytes", "s5gpu_refine_dev", "s5gpu_refine_batch"]


def test_library_exports_the_refine_calls_and_the_tool_is_built(tmp_path):
    from slow5tools_amd import _lib, build, refine

    build.build()
    assert os.access(refine.S5REFINE, os.X_OK)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    header = open(os.path.join(ROOT, "include", "slow5gpu.h")).read()
    assert not [s for s in _lib.EXPORTS if s + "(" not in header]          # _lib.EXPORTS is a subset of slow5gpu.h, still
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [15, 16, 2, 24, 19]
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   's5gpu_refine_params_t p = {0.5, 2.0, 64.0, 127, 16, 16, 2};\ns5gpu_fit_t f;\n'
                   'int (*a)(uint32_t, const int16_t *, uint32_t, const uint32_t *, const int16_t *, uint32_t, const int32_t *, const int32_t *, const int32_t *,'
                   ' uint32_t, const s5gpu_refine_params_t *, s5gpu_fit_t *, int16_t *, int32_t *, void *) = s5gpu_path_fit_dev;\n'
                   'int (*b)(uint32_t, const int16_t *, uint32_t, const uint32_t *, const int16_t *, uint32_t, const s5gpu_map_row_t *, uint32_t, uint32_t, void *,'
                   ' size_t, s5gpu_map_row_t *, int32_t *, int32_t *, int32_t *, void *) = s5gpu_sdtw_window_dev;\n'
                   'printf("%d %d %d %d %d %d\\n", S5GPU_STATUS_FIT_FLAT, S5GPU_STATUS_FIT_RANGE, (int)sizeof p, (int)sizeof f, a && b, (int)p.iters);return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == [str(FIT_FLAT), str(FIT_RANGE), "40", "64", "1", "2"]
    assert (_lib.STATUS_FIT_FLAT, _lib.STATUS_FIT_RANGE) == (FIT_FLAT, FIT_RANGE) and refine.FIT == FIT
    assert L.s5gpu_refine_work_bytes(4, 0) == 0 and L.s5gpu_refine_work_bytes(4, 1025) == 0 and L.s5gpu_refine_work_bytes(4, 64) % 16 == 0
    assert L.s5gpu_refine_work_bytes(5, 64) > L.s5gpu_refine_work_bytes(4, 64) >= 4 * (16 + 64 + 8 + 64 * 10)


def test_restatement_known_answers():
    """r[j] = 2 q[i] + 3 on a diagonal path: exactly a = 2, b = 3; a constant query: FIT_FLAT; a slope of 0.4: FIT_RANGE; a refused fit leaves
    every output of the rounds a copy of the input"""
    rng = np.random.default_rng(1)
    P = params()
    q = rng.integers(-40, 41, 50).astype(np.int16)
    r = np.concatenate([[120, -120, 120], 2 * q.astype(np.int64) + 3, [-120, 120]]).astype(np.int16)
    lo = hi = np.arange(3, 53, dtype=np.int32)
    st, fit = fit_ref(q, r, lo, hi, P)
    assert st == 0 and fit[0] == 2.0 and fit[1] == 3.0 and fit[2] == 50
    assert np.array_equal(requant_ref(q, fit[0], fit[1], 127), np.clip(r[3:53], -127, 127))
    # the rounds: the refined query is the slice itself, cost 0 in place
    got = refine_ref(q, r, (int(np.abs(q - r[3:53]).sum()), 50, 3, 52), lo, hi, 0, 1 << 20, P)
    assert got["status"] == 0 and got["rounds"] == 2 and got["row"] == (0, 50, 3, 52) and got["fit"][:2] == (2.0, 3.0)
    # half to even, the clamp, and the product rounded before the sum
    assert requant_ref([1, 3, -1, 100, -100], 0.5, 0.0, 127).tolist() == [0, 2, 0, 50, -50]
    assert requant_ref([100, -100], 2.0, 0.0, 127).tolist() == [127, -127]
    # a constant query: den = 0
    flat = np.full(50, 7, dtype=np.int16)
    st, fit = fit_ref(flat, r, lo, hi, P)
    assert st == FIT_FLAT and fit[:2] == (1.0, 0.0) and fit[2] == 50
    # too few cells
    assert fit_ref(q[:15], r, lo[:15], hi[:15], P)[0] == FIT_FLAT and fit_ref(q[:16], r, lo[:16], hi[:16], P)[0] == 0
    # r = 0.4 q: a slope of 0.4
    q5 = (5 * rng.integers(-20, 21, 50)).astype(np.int16)
    r5 = np.concatenate([[120, -120, 120], 2 * (q5.astype(np.int64) // 5), [-120, 120]]).astype(np.int16)
    st, fit = fit_ref(q5, r5, lo, hi, P)
    assert st == FIT_RANGE and fit[:2] == (1.0, 0.0)
    assert fit_ref(q5, r5, lo, hi, params(a_min=0.25))[0] == 0 and fit_ref(q5, r5, lo, hi, params(a_min=0.25))[1][0] == 0.4
    # |b| above b_max
    assert fit_ref(q, (r.astype(np.int64) + 100).astype(np.int16), lo, hi, P)[0] == FIT_RANGE
    for qq, rr, want in ((flat, r, FIT_FLAT), (q5, r5, FIT_RANGE)):
        row = (12345, 50, 3, 52)
        got = refine_ref(qq, rr, row, lo, hi, 0, 1 << 20, P)
        assert got["status"] == want and got["rounds"] == 0 and got["row"] == row and got["fit"] == FIT_NONE
        assert np.array_equal(got["q"], qq) and np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi)
    # a read with a status, a broken path, a span above wmax: no result at all
    assert refine_ref(q, r, (0, 50, 3, 52), lo, hi, QUERY_SHORT, 1 << 20, P)["status"] == QUERY_SHORT
    bad = lo.copy()
    bad[7] += 2
    got = refine_ref(q, r, (0, 50, 3, 52), bad, bad, 0, 1 << 20, P)
    assert got["status"] == PATH_ROW and got["row"] == EMPTY and not got["q"].any() and (got["lo"] == -1).all()
    assert refine_ref(q, r, (0, 50, 3, 52), lo, hi, 0, 49, P)["status"] == PATH_WIDE
    # the window: clipped at both ends, and one column too wide
    assert window_ref(q, r, (0, 50, 3, 52), 64, 55)[0] == 0 and window_ref(q, r, (0, 50, 3, 52), 64, 54)[0] == PATH_WIDE
    assert window_ref(q, r, (0, 50, 3, 52), 1, 52)[0] == 0 and window_ref(q, r, (0, 50, 3, 52), 1, 51)[0] == PATH_WIDE
    assert window_ref(q, r, (0, 49, 3, 52), 1, 52)[0] == PATH_ROW and window_ref(q, r, (0, 50, 3, 55), 1, 52)[0] == PATH_ROW


REFINE_HOST = r'''
// The code of k_path_fit, k_sdtw_win and k_sdtw_trace_win that lives in refine_dev.h and dtw_dev.h, on the CPU.  A case of in.bin: Q, R, G, pad,
// wmax, the row (qlen, start, end), the parameters, q0[Q], r[R], lo[Q], hi[Q].  The fit runs along lo / hi; q' is aligned in the window around the row:
// 64 lanes in lockstep, the words written the way the kernel lays them out into a slot of exactly the slot's size filled with ones, the
// candidate of the lane that holds row Q - 1, then the header's walk.  out.bin gets st_fit, the fit, q'[Q], st_win, cost', start', end',
// lo'[Q], hi'[Q] of each.
#define S5_REFINE_HOST
#include "refine_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace dtwk;
using namespace refk;
static void shift_up1(const uint32_t *v, uint32_t fill, uint32_t *out) { for (int l = 63; l >= 1; l--) out[l] = v[l - 1]; out[0] = fill; }

template <int G, int KB>
static U4 win(const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t W, uint32_t ws, uint32_t *slot, uint32_t slot_words) {
    const uint32_t SPW = 16 / G;
    std::vector<Lane<G, false> > L(64);
    uint32_t rcur[64], v[64], r[64], up[64], word[64];
    for (uint32_t l = 0; l < 64; l++) {
        lane_init(L[l], l == 0);
        rcur[l] = 0;
        for (int k = 0; k < G; k++) { const uint32_t row = l * G + k; L[l].q[k] = biased(row < Q ? q[row] : (int16_t)0); }
    }
    const uint32_t last = (Q - 1) / G;
    uint32_t nw = path_words(G, W + last);
    if (nw > slot_words) abort();
    for (uint32_t w = 0; w < nw; w++) {
        for (int l = 0; l < 64; l++) word[l] = 0;
        for (uint32_t s = 0; s < SPW; s++) {
            const uint32_t t = w * SPW + s;
            shift_up1(rcur, biased(t < W ? ref[t] : (int16_t)0), r);
            for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
            shift_up1(v, 0u, up);
            for (uint32_t l = 0; l < 64; l++) {
                word[l] = path_pack(word[l], lane_step_dirs(L[l], r[l], up[l]), s, G);
                lane_best<G, false, KB>(L[l], t - l, W);
            }
        }
        for (int l = 0; l < 64; l++) slot[(size_t)w * 64 + l] = word[l];
    }
    return result_row(L[last].best, Q, -1, (int32_t)ws + L[last].best_end);
}
template <int G, int KB = 0>
struct Pick {
    static U4 go(int kb, const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t W, uint32_t ws, uint32_t *slot, uint32_t slot_words) {
        if (kb == KB) return win<G, KB>(q, Q, ref, W, ws, slot, slot_words);
        if constexpr (KB + 1 < G) return Pick<G, KB + 1>::go(kb, q, Q, ref, W, ws, slot, slot_words);
        abort();
    }
};

static int one_case(FILE *f, FILE *o) {
    uint32_t h[5];
    int32_t se[3];                                                         // the row: qlen, start, end
    s5gpu_refine_params_t P;
    if (fread(h, 4, 5, f) != 5) return 1;
    const uint32_t Q = h[0], R = h[1], G = h[2], pad = h[3], wmax = h[4];
    if (fread(se, 4, 3, f) != 3 || fread(&P, sizeof P, 1, f) != 1 || Q < 1 || Q > 64 * G || R < 1 || !params_ok(P) || wmax < 1 || wmax > WMAX) return -1;
    std::vector<int16_t> q(Q), r(R), q1(Q, 0);
    std::vector<int32_t> lo(Q), hi(Q), lo1(Q, -1), hi1(Q, -1);
    if (fread(q.data(), 2, Q, f) != Q || fread(r.data(), 2, R, f) != R || fread(lo.data(), 4, Q, f) != Q || fread(hi.data(), 4, Q, f) != Q) return -1;
    // k_path_fit
    bool ok = true;
    for (uint32_t i = 0; i < Q; i++) ok = ok && pilek::row_ok(i, lo[i], hi[i], i ? hi[i - 1] : 0, R);
    int32_t st = !ok ? S5GPU_STATUS_PATH_ROW : (int64_t)hi[Q - 1] - (int64_t)lo[0] + 1 > (int64_t)wmax ? S5GPU_STATUS_PATH_WIDE : 0;
    const bool path = st == 0;
    s5gpu_fit_t F = fit_none();
    if (path) {
        Sums S = {0, 0, 0, 0, 0, 0};
        for (uint32_t i = 0; i < Q; i++) row_sums(lo[i], hi[i], q[i], r.data(), R, wmax, S);
        st = fit_solve(S, P, &F.a, &F.b);
        F.n = S.n; F.sq = S.sq; F.sr = S.sr; F.sqq = S.sqq; F.sqr = S.sqr; F.srr = S.srr;
        for (uint32_t i = 0; i < Q; i++) q1[i] = st == 0 ? requant_one(q[i], F.a, F.b, P.clip) : q[i];
    }
    fwrite(&st, 4, 1, o);
    fwrite(&F, sizeof F, 1, o);
    fwrite(q1.data(), 2, Q, o);
    // k_sdtw_win and k_sdtw_trace_win on q'
    U4 row = result_row(NO_COST, 0, -1, -1);
    int32_t sw = st;
    if (path) {
        uint32_t ws, W;
        sw = win_row_check(result_row(0, (uint32_t)se[0], se[1], se[2]), Q, R, pad, wmax, &ws, &W);
        if (sw == 0) {
            const uint32_t slot_words = path_words(G, wmax + 63);
            uint32_t *slot = (uint32_t *)malloc((size_t)slot_words * 256);
            if (!slot) return -1;
            memset(slot, 0xFF, (size_t)slot_words * 256);
            const int kb = (int)((Q - 1) % G);
            const int16_t *wref = r.data() + ws;
            if (G == 1) row = Pick<1>::go(kb, q1.data(), Q, wref, W, ws, slot, slot_words);
            else if (G == 2) row = Pick<2>::go(kb, q1.data(), Q, wref, W, ws, slot, slot_words);
            else if (G == 4) row = Pick<4>::go(kb, q1.data(), Q, wref, W, ws, slot, slot_words);
            else if (G == 8) row = Pick<8>::go(kb, q1.data(), Q, wref, W, ws, slot, slot_words);
            else if (G == 16) row = Pick<16>::go(kb, q1.data(), Q, wref, W, ws, slot, slot_words);
            else return -1;
            int32_t start = -1;
            const uint32_t jend = row.w - ws;
            sw = S5GPU_STATUS_PATH_ROW;
            if (jend < W) sw = path_walk_from(slot, slot_words, G, Q, W, (int32_t)ws, jend, lo1.data(), hi1.data(), &start);
            row.z = (uint32_t)start;
            free(slot);
        }
    }
    const int32_t head[4] = {sw, (int32_t)row.x, (int32_t)row.z, (int32_t)row.w};
    fwrite(head, 4, 4, o);
    fwrite(lo1.data(), 4, Q, o);
    fwrite(hi1.data(), 4, Q, o);
    return 0;
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


def scaled_read(rng, Q, R, where="mid", a=1.7, b=30.0):
    """a reference of R levels and a query of Q rows that is a piece of it seen through another scale: the piece's levels, each held 1 to 3
    times, put through (x - b) / a plus a little noise.  where: the piece starts at column 0, ends at column R - 1, or lies inside."""
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    S = max(1, min(R - 4, (Q + 1) // 2))
    s = {"left": 0, "right": R - S, "mid": int(rng.integers(1, R - S))}[where]
    counts = np.full(S, Q // S)
    counts[:Q % S] += 1
    lv = np.repeat(ref[s:s + S].astype(np.float64), counts)
    q = np.clip(np.rint((lv - b) / a + rng.normal(0.0, 0.7, Q)), -127, 127).astype(np.int16)
    return q, ref


def host_cases():
    """-> [(q, r, G, pad, wmax, row, lo, hi, params)]: every Q of QLENS with scaled reads (fits that are accepted) and tie-dense {-1, 0, 1}
    inputs (fits that are refused), pads 0, 1, 64, windows clipped at column 0 and at R - 1, W' = wmax and wmax + 1"""
    rng = np.random.default_rng(29)
    cases = []
    for k, Q in enumerate(QLENS):
        R = int(rng.integers(Q // 2 + 70, Q // 2 + 140))
        where = ("mid", "left", "right")[k % 3]
        for q, r in (scaled_read(rng, Q, R, where), (rng.integers(-1, 2, Q).astype(np.int16), rng.integers(-1, 2, R).astype(np.int16))):
            c, lo, hi = path_ref(q, r, cross_check=False)
            row = (c, Q, int(lo[0]), int(hi[-1]))
            for pad in PADS:
                W = min(R - 1, row[3] + pad) - max(0, row[2] - pad) + 1
                cases.append((q, r, _g_of(Q), pad, 1 << 20 if pad != 1 else W, row, lo, hi, params(pad=pad)))     # (pad 1: W' = wmax exactly)
                if pad == 1 and W > 1:
                    cases.append((q, r, _g_of(Q), pad, W - 1, row, lo, hi, params(pad=pad)))                       # W' = wmax + 1
    q, r = scaled_read(rng, 5, 70)
    c, lo, hi = path_ref(q, r)
    cases.append((q, r, 4, 64, 1 << 20, (c, 5, int(lo[0]), int(hi[-1])), lo, hi, params(pad=64, min_cells=2)))        # a G above the smallest
    q, r = scaled_read(rng, 100, 120)
    c, lo, hi = path_ref(q, r)
    row = (c, 100, int(lo[0]), int(hi[-1]))
    cases.append((q, r, 2, 3, 1 << 20, row, lo, hi, params(pad=3, a_min=1.9, a_max=1.95)))                            # refused: q' is q
    bad = lo.copy()
    bad[50] += 2
    cases.append((q, r, 2, 3, 1 << 20, row, bad, np.maximum(hi, bad), params(pad=3)))                                 # a gap of 2
    cases.append((q, r, 2, 3, 1 << 20, (c, 99, row[2], row[3]), lo, hi, params(pad=3)))                               # a row that is not the query's
    return cases


def _want_case(case):
    q, r, g, pad, wmax, row, lo, hi, P = case
    return round_ref(q, r, row, lo, hi, wmax, P)


def _build_refine_host(tmp_path, extra=()):
    return host_build(tmp_path, "refine_host", REFINE_HOST, ["-O1", "-std=c++17", "-ffp-contract=off"], extra)


def write_host_cases(path, cases):
    with open(path, "wb") as fh:
        for q, r, g, pad, wmax, row, lo, hi, P in cases:
            fh.write(struct.pack("<IIIIIiii", len(q), len(r), g, pad, wmax, row[1], row[2], row[3]) + params_bytes(P) + np.asarray(q, dtype=np.int16).tobytes()
                     + np.asarray(r, dtype=np.int16).tobytes() + np.asarray(lo, dtype=np.int32).tobytes() + np.asarray(hi, dtype=np.int32).tobytes())


def test_the_refine_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """row_sums, fit_solve, requant_one, win_row_check of refine_dev.h and lane_step_dirs, lane_best, path_walk_from of dtw_dev.h as g++
    compiles them, on host_cases()"""
    cases = host_cases()
    exe = _build_refine_host(tmp_path)
    write_host_cases(tmp_path / "in.bin", cases)
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw, at = (tmp_path / "out.bin").read_bytes(), 0
    seen, clipped = set(), set()
    for case in cases:
        q, r, g, pad, wmax, row, lo, hi, P = case
        Q = len(q)
        sf = int(np.frombuffer(raw, np.int32, 1, at)[0])
        fit = tuple(np.frombuffer(raw, FIT, 1, at + 4)[0].tolist())
        q1 = np.frombuffer(raw, np.int16, Q, at + 68)
        sw, cost, start, end = np.frombuffer(raw, np.int32, 4, at + 68 + 2 * Q).tolist()
        lo1, hi1 = np.frombuffer(raw, np.int32, Q, at + 84 + 2 * Q), np.frombuffer(raw, np.int32, Q, at + 84 + 6 * Q)
        at += 84 + 10 * Q
        wf, wfit, wq, wsw, wrow, wlo, whi = _want_case(case)
        what = (Q, len(r), g, pad, wmax)
        assert (sf, fit) == (wf, tuple(wfit)), what
        assert np.array_equal(q1, wq), what
        assert (sw, cost & 0xFFFFFFFF, start, end) == (wsw, wrow[0], wrow[2], wrow[3]), what
        assert np.array_equal(lo1, wlo) and np.array_equal(hi1, whi), what
        seen.add((sf, sw))
        if sw == 0 and pad:
            clipped |= {"left"} if row[2] - pad < 0 else set()
            clipped |= {"right"} if row[3] + pad > len(r) - 1 else set()
    assert at == len(raw)
    assert {(0, 0), (FIT_RANGE, 0), (0, PATH_WIDE), (PATH_ROW, PATH_ROW), (0, PATH_ROW)} <= seen and clipped == {"left", "right"}
    assert any(s[0] == FIT_FLAT or s[0] == FIT_RANGE for s in seen)


def test_the_planted_case():
    """§4.20's planted case in the restatement, two rounds with the defaults: (1) every read whose first mapping overlaps its true span and
    whose fit stays in range has a refined cost of at most a third of the first cost and refined ends within 1 column of the truth; (2)
    every read whose slope leaves [0.5, 2] comes back unchanged with FIT_RANGE; (3) at least half of the reads are of the first kind."""
    ref, reads = planted_refined(PLANTED_SEED)
    first_kind = 0
    for q, (s, e), (c, lo, hi), got in reads:
        overlaps = lo[0] <= e and hi[-1] >= s
        if got["status"] == FIT_RANGE:
            assert got["rounds"] == 0 and got["row"] == (c, len(q), lo[0], hi[-1]) and np.array_equal(got["q"], q)
            assert np.array_equal(got["lo"], lo) and np.array_equal(got["hi"], hi) and got["fit"] == FIT_NONE
        elif overlaps and got["status"] == 0:
            first_kind += 1
            assert got["rounds"] == 2
            assert 3 * got["row"][0] <= c, (s, e, c, got["row"])
            assert abs(got["row"][2] - s) <= 1 and abs(got["row"][3] - e) <= 1, (s, e, got["row"])
    assert 2 * first_kind >= len(reads)


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3): the pointers are never dereferenced on the host, so made-up aligned addresses serve"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    A = 1 << 20                                                            # an aligned address
    nan, inf = float("nan"), float("inf")
    bad_params = [dict(a_min=0.0), dict(a_min=-1.0), dict(a_min=nan), dict(a_min=3.0), dict(a_max=inf), dict(a_max=nan), dict(b_max=inf), dict(b_max=nan),
                  dict(b_max=-1.0), dict(clip=0), dict(clip=32768), dict(pad=65536), dict(min_cells=1), dict(min_cells=0), dict(iters=0), dict(iters=5)]

    def fit(n=4, q=A, pitch=64, ql=A, ref=A, R=100, lo=A, hi=A, si=A, wmax=256, P=None, pnull=False, fo=A, qo=A, so=A):
        p = c_params(P or params())
        return L.s5gpu_path_fit_dev(n, q, pitch, ql, ref, R, lo, hi, si, wmax, None if pnull else C.byref(p), fo, qo, so, None)
    assert fit(pitch=0) == -1 and fit(pitch=1025) == -1 and fit(R=0) == -1 and fit(R=1 << 31) == -1 and fit(ref=None) == -1
    assert fit(wmax=0) == -1 and fit(wmax=(1 << 20) + 1) == -1 and fit(pnull=True) == -1
    for kw in bad_params:
        assert fit(P=params(**kw)) == -1, kw
    for name in ("q", "ql", "lo", "hi", "si", "fo", "so"):
        assert fit(**{name: None}) == -1, name
    assert fit(q=A + 1) == -1 and fit(ql=A + 2) == -1 and fit(ref=A + 1) == -1 and fit(lo=A + 2) == -1 and fit(hi=A + 1) == -1 and fit(si=A + 2) == -1
    assert fit(fo=A + 8) == -1 and fit(qo=A + 1) == -1 and fit(so=A + 2) == -1
    assert fit(n=0) == 0 and fit(n=0, q=None, fo=None) == 0               # nothing to do: nothing is launched

    def win(n=4, q=A, pitch=64, ql=A, ref=A, R=100, rows=A, pad=16, wmax=256, scratch=A, sb=1 << 30, ro=2 * A, lo=A, hi=A, st=A):
        return L.s5gpu_sdtw_window_dev(n, q, pitch, ql, ref, R, rows, pad, wmax, scratch, sb, ro, lo, hi, st, None)
    assert win(pitch=0) == -1 and win(pitch=1025) == -1 and win(R=0) == -1 and win(R=1 << 31) == -1 and win(ref=None) == -1
    assert win(wmax=0) == -1 and win(wmax=(1 << 20) + 1) == -1 and win(pad=65536) == -1 and win(ro=A) == -1
    for name in ("q", "ql", "rows", "scratch", "ro", "lo", "hi", "st"):
        assert win(**{name: None}) == -1, name
    assert win(q=A + 1) == -1 and win(ql=A + 2) == -1 and win(rows=A + 8) == -1 and win(scratch=A + 8) == -1 and win(ro=2 * A + 8) == -1
    assert win(lo=A + 2) == -1 and win(hi=A + 1) == -1 and win(st=A + 2) == -1
    slot = L.s5gpu_sdtw_path_slot_bytes(64, 256)
    assert win(sb=slot - 1) == -3 and win(sb=0) == -3 and win(n=0) == 0 and win(n=0, sb=0) == 0

    def rounds(n=4, q=A, pitch=64, ql=A, ref=A, R=100, rows=A, lo=A, hi=A, si=A, wmax=256, P=None, scratch=A, sb=1 << 30, work=A, wb=1 << 30, qo=2 * A, ro=2 * A,
               lo2=2 * A, hi2=2 * A, fo=A, so=2 * A, rn=A):
        p = c_params(P or params())
        return L.s5gpu_refine_dev(n, q, pitch, ql, ref, R, rows, lo, hi, si, wmax, C.byref(p), scratch, sb, work, wb, qo, ro, lo2, hi2, fo, so, rn, None)
    assert rounds(pitch=0) == -1 and rounds(R=0) == -1 and rounds(ref=None) == -1 and rounds(wmax=0) == -1
    for kw in bad_params:
        assert rounds(P=params(**kw)) == -1, kw
    for name in ("q", "ql", "rows", "lo", "hi", "si", "scratch", "work", "qo", "ro", "lo2", "hi2", "fo", "so", "rn"):
        assert rounds(**{name: None}) == -1, name
    assert rounds(rows=A + 8) == -1 and rounds(work=A + 8) == -1 and rounds(fo=A + 8) == -1 and rounds(rn=A + 2) == -1 and rounds(qo=2 * A + 1) == -1
    assert rounds(qo=A) == -1 and rounds(ro=A) == -1 and rounds(lo2=A) == -1 and rounds(so=A) == -1                  # an output that is an input
    assert rounds(wb=L.s5gpu_refine_work_bytes(4, 64) - 1) == -3 and rounds(sb=slot - 1) == -3 and rounds(n=0) == 0
    # the batch call: the cases of s5gpu_align_batch, the parameters, the outputs
    vp = C.c_void_p
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    h_rows, h_rows2, h_fit = np.full(16, 0xA5, dtype=np.uint8), np.full(16, 0xA5, dtype=np.uint8), np.full(64, 0xA5, dtype=np.uint8)
    h_lo, h_hi, h_st = np.full(64, -7, dtype=np.int32), np.full(64, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)

    def batch(pr=(0, 64, 10, 32.0, 127, 1), ev=DNA, wmax=256, R=100, ref=True, P=None, pnull=False, rows=True, rows2=True, fo=True, lo=True, methods=(1, 1)):
        e, p, rp = _lib.EventParams(*ev), _lib.MapParams(*pr), c_params(P or params())
        return L.s5gpu_refine_batch(1, rec_p, rl, methods[0], methods[1], C.byref(e), C.byref(p), wmax, None if pnull else C.byref(rp),
                                    h_ref.ctypes.data_as(vp) if ref else None, R, h_rows.ctypes.data_as(vp) if rows else None,
                                    h_rows2.ctypes.data_as(vp) if rows2 else None, h_fit.ctypes.data_as(vp) if fo else None,
                                    h_lo.ctypes.data_as(vp) if lo else None, h_hi.ctypes.data_as(vp), None, h_st.ctypes.data_as(vp), None)
    for pr in ((0, 0, 1, 32.0, 127, 1), (0, 1025, 1, 32.0, 127, 1), (0, 64, 0, 32.0, 127, 1), (0, 64, 10, nan, 127, 1), (0, 64, 10, 32.0, 0, 1)):
        assert batch(pr=pr) == -1, pr
    assert batch(wmax=0) == -1 and batch(wmax=(1 << 20) + 1) == -1 and batch(R=0) == -1 and batch(ref=False) == -1 and batch(pnull=True) == -1
    assert batch(rows=False) == -1 and batch(rows2=False) == -1 and batch(fo=False) == -1 and batch(lo=False) == -1 and batch(methods=(9, 1)) == -1
    for kw in bad_params:
        assert batch(P=params(**kw)) == -1, kw
    assert (h_rows == 0xA5).all() and (h_rows2 == 0xA5).all() and (h_fit == 0xA5).all() and (h_lo == -7).all() and (h_hi == -7).all() and (h_st == -7).all()


# ---------------------------------------------------------------------------------------------------------------- gpu

class Batch:
    """queries [n, pitch], qlen and a reference, and what the device makes of them with s5gpu_sdtw_dev and s5gpu_sdtw_path_dev, on both sides"""

    def __init__(self, env, qm, qlens, ref):
        self.qm, self.ql, self.ref = np.ascontiguousarray(qm, dtype=np.int16), np.asarray(qlens, dtype=np.int32), np.ascontiguousarray(ref, dtype=np.int16)
        self.n, self.pitch, self.R = len(self.ql), self.qm.shape[1], len(self.ref)
        self.d_q, self.d_ql, self.d_r = to_dev(env, self.qm), to_dev(env, self.ql), to_dev(env, self.ref)
        self.d_rows = env.map.sdtw_dev(self.d_q, self.d_ql, self.d_r, want_start=True)
        self.d_lo, self.d_hi, self.d_st = env.align.path_dev(self.d_q, self.d_ql, self.d_r, self.d_rows, wmax=self.R)
        env.torch.cuda.synchronize()
        self.rows = self.d_rows.cpu().numpy().view(MAP_ROW).reshape(-1).copy()
        self.lo, self.hi, self.st = self.d_lo.cpu().numpy().copy(), self.d_hi.cpu().numpy().copy(), self.d_st.cpu().numpy().copy()
        assert not self.st.any()


def _mixed_batch(env, R):
    """the Q list twice, scaled reads and tie-dense ones, on a reference of R levels"""
    rng = np.random.default_rng(300 + R)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    qm = np.full((2 * len(QLENS), 1024), 9999, dtype=np.int16)
    for i, Q in enumerate(QLENS):
        S = max(1, min(R - 4, (Q + 1) // 2))
        s = int(rng.integers(0, R - S + 1)) if i % 3 else (0 if i % 2 else R - S)
        counts = np.full(S, Q // S)
        counts[:Q % S] += 1
        lv = np.repeat(ref[s:s + S].astype(np.float64), counts)
        qm[i, :Q] = np.clip(np.rint((lv - 30.0) / 1.7 + rng.normal(0.0, 0.7, Q)), -127, 127)
        qm[len(QLENS) + i, :Q] = rng.integers(-1, 2, Q)
    if R == 129:
        ref = np.where(np.arange(R) % 2 == 0, ref, rng.integers(-1, 2, R)).astype(np.int16)
    return Batch(env, qm, QLENS + QLENS, ref)


@pytest.fixture(scope="module")
def mixed(gpu):
    return {R: _mixed_batch(gpu, R) for R in (65, 129, 500)}


def _run_fit(env, B, lo, hi, st_in, wmax, P, want_queries=True):
    """s5gpu_path_fit_dev with guard words around every output -> (fit [n] FIT, q' [n, pitch], status)"""
    torch, L = env.torch, env.L
    n, pitch = B.n, B.pitch
    d_lo, d_hi, d_si = to_dev(env, lo, np.int32), to_dev(env, hi, np.int32), to_dev(env, st_in, np.int32)
    d_fit = torch.full(((n + 2) * 16,), GUARD, dtype=torch.int32, device="cuda")
    d_qo = torch.full(((n + 2) * pitch,), 0x5A5A, dtype=torch.int16, device="cuda")
    d_so = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda")
    p = c_params(P)
    rc = L.s5gpu_path_fit_dev(n, B.d_q.data_ptr(), pitch, B.d_ql.data_ptr(), B.d_r.data_ptr(), B.R, d_lo.data_ptr(), d_hi.data_ptr(), d_si.data_ptr(), wmax,
                              C.byref(p), d_fit.data_ptr() + 64, d_qo.data_ptr() + 2 * pitch if want_queries else None, d_so.data_ptr() + 4, None)
    torch.cuda.synchronize()
    assert rc == 0
    fit, qo, so = d_fit.cpu().numpy(), d_qo.cpu().numpy(), d_so.cpu().numpy()
    assert (fit[:16] == GUARD).all() and (fit[-16:] == GUARD).all() and (so[[0, -1]] == GUARD).all(), "a guard word was written"
    assert (qo[:pitch] == 0x5A5A).all() and (qo[-pitch:] == 0x5A5A).all() and (want_queries or (qo == 0x5A5A).all()), "a guard word was written"
    assert np.array_equal(d_lo.cpu().numpy(), lo) and np.array_equal(d_hi.cpu().numpy(), hi) and np.array_equal(B.d_q.cpu().numpy(), B.qm)
    return fit[16:-16].view(FIT).reshape(-1).copy(), qo[pitch:-pitch].reshape(n, pitch).copy(), so[1:-1].copy()


def _want_fit(B, lo, hi, st_in, wmax, P):
    fit, qo, so = np.zeros(B.n, dtype=FIT), np.zeros((B.n, B.pitch), dtype=np.int16), np.zeros(B.n, dtype=np.int32)
    for i in range(B.n):
        Q = min(int(B.ql[i]), B.pitch)
        fit[i], so[i] = FIT_NONE, st_in[i]
        if st_in[i] != 0 or Q == 0:
            continue
        st = path_status_ref(lo[i, :Q], hi[i, :Q], B.R, wmax)
        if st == 0:
            st, f = fit_ref(B.qm[i, :Q], B.ref, lo[i, :Q], hi[i, :Q], P)
            fit[i] = f
            qo[i, :Q] = requant_ref(B.qm[i, :Q], f[0], f[1], P["clip"]) if st == 0 else B.qm[i, :Q]
        so[i] = st
    return fit, qo, so


@pytest.mark.gpu
@pytest.mark.parametrize("R", [65, 129, 500])
def test_fit_is_exact_on_a_mixed_batch(gpu, mixed, R):
    """the sums, a and b as the same doubles, q' and the status, byte for byte: the Q list, paths from s5gpu_sdtw_path_dev, reads with an
    incoming status, a span above wmax, hand-broken rows"""
    B = mixed[R]
    P = params()
    lo, hi, st_in = B.lo.copy(), B.hi.copy(), np.zeros(B.n, dtype=np.int32)
    spans = B.rows["end"] - B.rows["start"] + 1
    wmax = int(np.unique(np.delete(spans, [2, 4, 5, 6, 13, len(QLENS) + 7]))[-2])      # the widest of the other paths are above it, one at least meets it
    st_in[[2, 13]] = [QUERY_SHORT, 4]
    k = len(QLENS)
    lo[4, 10], hi[4, 10] = hi[4, 10] + 1, lo[4, 10]                        # lo > hi
    hi[5, int(B.ql[5]) - 1] = R                                            # hi >= R
    lo[6, 20:int(B.ql[6])] += 2                                            # a gap of 2
    hi[6, 20:int(B.ql[6])] += 2
    hi[6] = np.minimum(hi[6], R - 1)
    lo[6] = np.minimum(lo[6], hi[6])
    lo[k + 7, 0] = -1                                                      # lo < 0
    want = _want_fit(B, lo, hi, st_in, wmax, P)
    assert {0, QUERY_SHORT, 4, PATH_ROW, PATH_WIDE} <= set(want[2].tolist()) and (FIT_RANGE in want[2] or FIT_FLAT in want[2])
    assert (want[2] == 0).sum() >= 2 and (want[2] == PATH_ROW).sum() >= 4 and (want[2] == PATH_WIDE).sum() >= 1
    fit, qo, so = _run_fit(gpu, B, lo, hi, st_in, wmax, P)
    assert so.tolist() == want[2].tolist()
    assert fit.tobytes() == want[0].tobytes(), [(i, fit[i].tolist(), want[0][i].tolist()) for i in range(B.n) if fit[i] != want[0][i]][:3]
    assert np.array_equal(qo, want[1])
    # without queries_out, and with parameters that accept more and clamp lower
    P2 = params(a_min=0.01, a_max=50.0, b_max=500.0, clip=60, min_cells=2)
    want2 = _want_fit(B, lo, hi, st_in, int(spans.max()), P2)             # (and a wmax that no path is above)
    assert (want2[2] == 0).sum() > (want[2] == 0).sum() and PATH_WIDE not in want2[2] and not np.array_equal(want2[1], want[1])
    fit2, qo2, so2 = _run_fit(gpu, B, lo, hi, st_in, int(spans.max()), P2)
    assert so2.tolist() == want2[2].tolist() and fit2.tobytes() == want2[0].tobytes() and np.array_equal(qo2, want2[1]) and np.abs(qo2).max() <= 60 < np.abs(qo).max()
    fit3, _, so3 = _run_fit(gpu, B, lo, hi, st_in, wmax, P, want_queries=False)
    assert fit3.tobytes() == want[0].tobytes() and so3.tolist() == want[2].tolist()


def _run_window(env, B, rows, pad, wmax, scratch_bytes=None, expect=0):
    """s5gpu_sdtw_window_dev with guards around rows_out, lo, hi and status and behind the scratch -> (rows', lo, hi, status)"""
    torch, L = env.torch, env.L
    n, pitch = B.n, B.pitch
    d_rows = to_dev(env, np.ascontiguousarray(rows).view(np.int32).reshape(n, 4))
    slot = L.s5gpu_sdtw_path_slot_bytes(pitch, wmax)
    sb = slot * n if scratch_bytes is None else scratch_bytes
    d_scr = torch.full((sb // 4 + 64,), GUARD, dtype=torch.int32, device="cuda")
    d_ro = torch.full(((n + 2) * 4,), GUARD, dtype=torch.int32, device="cuda")
    d_lo = torch.full(((n + 2) * pitch,), GUARD, dtype=torch.int32, device="cuda")
    d_hi = torch.full(((n + 2) * pitch,), GUARD, dtype=torch.int32, device="cuda")
    d_st = torch.full((n + 2,), GUARD, dtype=torch.int32, device="cuda")
    rc = L.s5gpu_sdtw_window_dev(n, B.d_q.data_ptr(), pitch, B.d_ql.data_ptr(), B.d_r.data_ptr(), B.R, d_rows.data_ptr(), pad, wmax, d_scr.data_ptr(), sb,
                                 d_ro.data_ptr() + 16, d_lo.data_ptr() + 4 * pitch, d_hi.data_ptr() + 4 * pitch, d_st.data_ptr() + 4, None)
    torch.cuda.synchronize()
    assert rc == expect
    ro, lo, hi, st, scr = d_ro.cpu().numpy(), d_lo.cpu().numpy(), d_hi.cpu().numpy(), d_st.cpu().numpy(), d_scr.cpu().numpy()
    if rc != 0:
        assert (ro == GUARD).all() and (lo == GUARD).all() and (hi == GUARD).all() and (st == GUARD).all() and (scr == GUARD).all()
        return None
    for a, w in ((ro, 4), (lo, pitch), (hi, pitch), (st, 1)):
        assert (a[:w] == GUARD).all() and (a[-w:] == GUARD).all(), "a guard row was written"
    assert (scr[sb // 4:] == GUARD).all(), "the guard behind the scratch was written"
    return ro[4:-4].view(MAP_ROW).reshape(-1).copy(), lo[pitch:-pitch].reshape(n, pitch).copy(), hi[pitch:-pitch].reshape(n, pitch).copy(), st[1:-1].copy()


def _want_window(B, rows, pad, wmax):
    ro, lo, hi = np.zeros(B.n, dtype=MAP_ROW), np.full((B.n, B.pitch), -1, dtype=np.int32), np.full((B.n, B.pitch), -1, dtype=np.int32)
    st = np.zeros(B.n, dtype=np.int32)
    for i in range(B.n):
        Q = min(int(B.ql[i]), B.pitch)
        ro[i] = EMPTY
        if Q:
            st[i], ro[i], lo[i, :Q], hi[i, :Q] = window_ref(B.qm[i, :Q], B.ref, rows[i], pad, wmax)
    return ro, lo, hi, st


def _same(got, want, what):
    for name, g, w in zip(("rows", "lo", "hi", "status"), got, want):
        assert g.tolist() == w.tolist(), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("R", [65, 129, 500])
def test_window_is_exact_on_a_mixed_batch(gpu, mixed, R, pad):
    """rows', lo, hi and the status against path_ref on the slice: windows clipped at column 0 and at R - 1, W' = wmax and wmax + 1"""
    B = mixed[R]
    W = np.minimum(R - 1, B.rows["end"] + pad) - np.maximum(0, B.rows["start"] - pad) + 1
    widths = np.unique(np.delete(W, 3))
    wmax = int(widths[-2] if len(widths) > 1 else widths[-1])              # W' = wmax for one read at least; the widest windows are above it
    rows = B.rows.copy()
    rows[3]["qlen"] += 1                                                   # a row that is not the query's
    want = _want_window(B, rows, pad, wmax)
    assert (want[3] == PATH_WIDE).sum() >= (len(widths) > 1) and (want[3] == PATH_ROW).sum() == 1 and (want[3] == 0).sum() >= 4
    if pad == 64:
        assert (B.rows["start"] - pad < 0).any() and (B.rows["end"] + pad > R - 1).any()
    _same(_run_window(gpu, B, rows, pad, wmax), want, (R, pad))
    want = _want_window(B, rows, pad, int(W.max()))                        # every read in its window
    assert (want[3] == 0).sum() == B.n - 1
    _same(_run_window(gpu, B, rows, pad, int(W.max())), want, (R, pad, "all"))


@pytest.mark.gpu
def test_window_every_row_of_the_last_lane(gpu):
    qm, ql = last_lane_batch()
    B = Batch(gpu, qm, ql, np.random.default_rng(42).integers(-127, 128, 129).astype(np.int16))
    want = _want_window(B, B.rows, 1, 129)
    assert not want[3].any() and want[0]["qlen"].tolist() == ql and (want[0]["cost"] < 2 ** 26).all()          # every read has a result
    assert (want[1][:, 0] >= 0).all()
    _same(_run_window(gpu, B, B.rows, 1, 129), want, "every row of the last lane")


@pytest.mark.gpu
def test_window_in_groups_and_over_many_workgroups(gpu, mixed):
    B = mixed[129]
    wmax = 129
    whole = _run_window(gpu, B, B.rows, 1, wmax)
    _same(whole, _want_window(B, B.rows, 1, wmax), "ungrouped")
    slot = gpu.L.s5gpu_sdtw_path_slot_bytes(1024, wmax)
    for sb in (3 * slot, 3 * slot + 100, slot):                            # scratch for 3 slots: 7 groups, the last of 2 reads
        _same(_run_window(gpu, B, B.rows, 1, wmax, scratch_bytes=sb), whole, sb)
    assert _run_window(gpu, B, B.rows, 1, wmax, scratch_bytes=slot - 1, expect=-3) is None
    # 4 x 256 + 1 reads: many waves and workgroups
    rng = np.random.default_rng(12)
    n = 4 * 256 + 1
    ref = rng.integers(-127, 128, 65).astype(np.int16)
    qm = rng.integers(-127, 128, (n, 12)).astype(np.int16)
    M = Batch(gpu, qm, [12] * n, ref)
    got = _run_window(gpu, M, M.rows, 2, 65)
    _same(got, _want_window(M, M.rows, 2, 65), "n = 1025")
    assert len(set(got[0]["end"].tolist())) > 20


def _planted_batch(env):
    ref, reads = planted(PLANTED_SEED)
    pitch = 160
    qm = np.zeros((len(reads) + 1, pitch), dtype=np.int16)
    for i, (q, s, e) in enumerate(reads):
        qm[i, :len(q)] = q
    return Batch(env, qm, [len(q) for q, s, e in reads] + [0], ref)          # (and a read without a query)


def _want_refine(B, st_in, wmax, P):
    out = [refine_ref(B.qm[i, :B.ql[i]], B.ref, tuple(B.rows[i].tolist()), B.lo[i, :B.ql[i]], B.hi[i, :B.ql[i]], int(st_in[i]), wmax, P) for i in range(B.n)]
    q, lo, hi = np.zeros((B.n, B.pitch), dtype=np.int16), np.full((B.n, B.pitch), -1, dtype=np.int32), np.full((B.n, B.pitch), -1, dtype=np.int32)
    for i, o in enumerate(out):
        Q = int(B.ql[i])
        q[i, :Q], lo[i, :Q], hi[i, :Q] = o["q"], o["lo"], o["hi"]
    rows = np.array([o["row"] for o in out], dtype=MAP_ROW)
    fit = np.array([o["fit"] for o in out], dtype=FIT)
    return q, rows, lo, hi, fit, np.array([o["status"] for o in out], dtype=np.int32), np.array([o["rounds"] for o in out], dtype=np.int32)


def _got_refine(env, B, st_in, wmax, P, scratch_bytes=None):
    R = env.refine.refine_dev(B.d_q, B.d_ql, B.d_r, B.d_rows, B.d_lo, B.d_hi, to_dev(env, st_in, np.int32), wmax, c_params(P), scratch_bytes)
    env.torch.cuda.synchronize()
    return (R.queries.cpu().numpy(), R.rows.cpu().numpy().view(MAP_ROW).reshape(-1), R.lo.cpu().numpy(), R.hi.cpu().numpy(), R.fit.cpu().numpy().view(FIT).reshape(-1),
            R.status.cpu().numpy(), R.rounds.cpu().numpy())


def _same_refine(got, want, what):
    for name, g, w in zip(("queries", "rows", "lo", "hi", "fit", "status", "rounds"), got, want):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, name, [i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes()][:5])


@pytest.mark.gpu
def test_refine_rounds_equal_the_iterated_restatement_on_the_planted_case(gpu):
    B = _planted_batch(gpu)
    st_in = np.zeros(B.n, dtype=np.int32)
    st_in[5] = QUERY_SHORT
    for iters in (1, 3):
        P = params(iters=iters)
        want = _want_refine(B, st_in, 1 << 12, P)
        _same_refine(_got_refine(gpu, B, st_in, 1 << 12, P), want, iters)
        assert (want[6] == iters).sum() >= B.n // 2 and FIT_RANGE in want[5] and want[5][5] == QUERY_SHORT and want[6][-1] == 0
    # a read that is rejected in round 2 and keeps round 1: a wmax that its first window meets and its second, around the longer refined
    # span, does not (pad 2, so that the span decides)
    P = params(iters=3, pad=2)
    free = _want_refine(B, st_in, 1 << 12, params(iters=1, pad=2))
    grown = [i for i in range(B.n) if free[5][i] == 0 and free[6][i] == 1
             and free[1][i]["end"] - free[1][i]["start"] > B.rows[i]["end"] - B.rows[i]["start"]]
    assert grown
    i = grown[0]
    wmax = int(min(B.R - 1, B.rows[i]["end"] + 2) - max(0, B.rows[i]["start"] - 2) + 1)
    want = _want_refine(B, st_in, wmax, P)
    assert want[5][i] == PATH_WIDE and want[6][i] == 1 and want[1][i].tolist() == free[1][i].tolist()
    got = _got_refine(gpu, B, st_in, wmax, P)
    _same_refine(got, want, "wmax %d" % wmax)
    # in groups: scratch for 3 slots
    slot = gpu.L.s5gpu_sdtw_path_slot_bytes(B.pitch, wmax)
    _same_refine(_got_refine(gpu, B, st_in, wmax, P, scratch_bytes=3 * slot), want, "groups")


@pytest.mark.gpu
def test_refined_outputs_feed_the_pileup(gpu):
    """what refine_dev returns goes to pileup.accum_dev as it is; the table meets §4.18's invariants"""
    torch = gpu.torch
    B = _planted_batch(gpu)
    R = gpu.refine.refine_dev(B.d_q, B.d_ql, B.d_r, B.d_rows, B.d_lo, B.d_hi, B.d_st)
    acc = gpu.pileup.new_acc(B.R)
    gpu.pileup.accum_dev(R.queries, B.d_ql, B.d_r, R.lo, R.hi, R.status, acc)
    torch.cuda.synchronize()
    total, cols = gpu.pileup.to_host(acc)
    st, rows, lo, hi, q = R.status.cpu().numpy(), R.rows.cpu().numpy().view(MAP_ROW).reshape(-1), R.lo.cpu().numpy(), R.hi.cpu().numpy(), R.queries.cpu().numpy()
    used = (st == 0) & (B.ql > 0)
    assert used.sum() >= B.n // 2 and total["reads_used"] == used.sum() and total["reads_skipped"] == B.n - used.sum() and total["reads_bad"] == 0
    assert total["R"] == B.R and total["cells"] == cols["n_events"].sum() and total["cost"] == cols["sum_cost"].sum()
    assert total["cost"] == rows["cost"][used].astype(np.int64).sum()      # the refined paths add up to the refined costs
    depth, n_ev, sum_q = np.zeros(B.R, dtype=np.int64), np.zeros(B.R, dtype=np.int64), np.zeros(B.R, dtype=np.int64)
    for i in np.flatnonzero(used):
        depth[rows[i]["start"]:rows[i]["end"] + 1] += 1
        for k in range(int(B.ql[i])):
            n_ev[lo[i, k]:hi[i, k] + 1] += 1
            sum_q[lo[i, k]:hi[i, k] + 1] += int(q[i, k])
    assert np.array_equal(cols["depth"], depth) and np.array_equal(cols["n_events"], n_ev) and np.array_equal(cols["sum_q"], sum_q)
    empty = n_ev == 0
    assert (cols["min_q"][empty] == 32767).all() and (cols["max_q"][empty] == -32768).all() and (cols["min_q"][~empty] <= cols["max_q"][~empty]).all()


@pytest.mark.gpu
def test_refine_end_to_end_on_a_synthetic_file(gpu, tmp_path):
    """read_refine (s5gpu_refine_batch) and file_refine (s5refine) agree with refine_on on level signals, one record corrupt and one read too
    short; the reference is the reads' own levels seen through another scale, so that fits are accepted"""
    rf = gpu.refine
    rng = np.random.default_rng(43)
    lengths = [3000, 500, 40, 5000, 1500, 2500]
    sigs = [levels_signal(n, rng) for n in lengths]
    recs = [record(i, s) for i, s in enumerate(sigs)]
    bad = bytearray(recs[3])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[3] = bytes(bad)
    n, skip, qmax, qmin = len(recs), 2, 100, 20
    ids = [ob.synth_read_id(i) for i in range(n)]
    ids = [i if isinstance(i, bytes) else i.encode() for i in ids]
    # the reference: the event means of read 0 and read 4 (what the device makes of them), between stretches of other levels with another spread
    dec = gpu.press.decode_to_device(recs)
    ev_rows, first = gpu.events.events_dev(dec, DNA, "raw")
    h_ev, h_first = ev_rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    m0, m4 = h_ev["mean"][h_first[0]:h_first[1]][:130], h_ev["mean"][h_first[4]:h_first[5]][:90]
    levels = np.concatenate([rng.normal(620.0, 200.0, 120), m0, rng.normal(380.0, 80.0, 100), m4, rng.normal(500.0, 110.0, 80)]).astype(np.float32)
    ref = quant_ref(levels)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n" + "".join("%.9g\n" % v for v in levels))
    kw = dict(skip=skip, qmax=qmax, qmin=qmin)
    rows, want = rf.refine_on(dec, ref, **kw)
    assert want.status[2] == QUERY_SHORT and want.status[3] not in (0, QUERY_SHORT, PATH_WIDE, PATH_ROW, FIT_FLAT, FIT_RANGE)
    assert want.status[0] == 0 and want.rounds[0] == 2 and want.rows[0]["cost"] < rows[0]["cost"] and want.fit[0]["a"] != 1.0
    assert want.rows[2].tolist() == EMPTY and want.rows[3].tolist() == EMPTY and (want.lo[2] == -1).all() and want.rounds[2] == 0
    # the restatement on the first mapping of read 0
    dq, dql, _ = gpu.map.queries_dev(ev_rows, first, dec.t_fields.view(gpu.torch.int32).view(-1, 16)[:n, 0].contiguous(), skip, qmax, qmin)
    q0 = dq.cpu().numpy()[0, :int(dql[0])]
    c, lo, hi = path_ref(q0, ref, cross_check=False)
    assert rows[0].tolist() == (c, len(q0), lo[0], hi[-1])
    r0 = refine_ref(q0, ref, (c, len(q0), int(lo[0]), int(hi[-1])), lo, hi, 0, 4 * qmax, params())
    assert want.rows[0].tolist() == r0["row"] and np.array_equal(want.lo[0, :len(q0)], r0["lo"]) and tuple(want.fit[0].tolist()) == r0["fit"]
    # the batch call
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        rf.read_refine(recs, ref, **kw)
    b_rows, b_rows2, b_fit, b_lo, b_hi, b_ev, b_st, b_rounds = rf.read_refine(recs, ref, raise_on_error=False, **kw)
    assert b_rows.tolist() == rows.tolist() and b_rows2.tolist() == want.rows.tolist() and b_fit.tobytes() == want.fit.tobytes()
    assert np.array_equal(b_lo, want.lo) and np.array_equal(b_hi, want.hi) and b_st.tolist() == want.status.tolist() and b_rounds.tolist() == want.rounds.tolist()
    for i in range(n):
        ql = int(b_rows[i]["qlen"])
        assert b_ev[i, :ql].tobytes() == h_ev[h_first[i] + skip:h_first[i] + skip + ql].tobytes() and not b_ev[i, ql:].tobytes().strip(b"\0")
    # other parameters go through: one round, a slope range that refuses every fit
    p1 = rf.RefineParams(iters=1, a_min=1.0e-3, a_max=2.0e-3)
    _, w1 = rf.refine_on(dec, ref, params=p1, **kw)
    o1 = rf.read_refine(recs, ref, raise_on_error=False, params=p1, **kw)
    assert o1[1].tolist() == w1.rows.tolist() and o1[6].tolist() == w1.status.tolist() and set(w1.status[[0, 1, 4, 5]].tolist()) <= {FIT_RANGE, FIT_FLAT}
    assert o1[1][[0, 1, 4, 5]].tolist() == rows[[0, 1, 4, 5]].tolist() and not o1[7].any()
    # the tool: exit 1, the corrupt read named, the other reads' lines
    synth_file(tmp_path / "reads.blow5", recs)
    args = ["--skip", str(skip), "--events", str(qmax), "--min-events", str(qmin), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([rf.S5REFINE, "-K", "4"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[3] in p.stderr and b"short" in p.stderr, p.stderr
    keep = [0, 1, 2, 4, 5]
    names = {0: b"ok", FIT_FLAT: b"flat", FIT_RANGE: b"range", PATH_WIDE: b"wide"}
    lines = []
    for i in keep:
        if want.status[i] == QUERY_SHORT:
            lines.append(ids[i] + b"\t*" * 11 + b"\n")
            continue
        lines.append(b"%s\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % (
            ids[i], rows[i]["qlen"], rows[i]["cost"], rows[i]["start"], rows[i]["end"], b"%.9g" % want.fit[i]["a"], b"%.9g" % want.fit[i]["b"], want.rounds[i],
            want.rows[i]["cost"], want.rows[i]["start"], want.rows[i]["end"], names[int(want.status[i])]))
    assert p.stdout == b"".join(lines)
    fids, flines = rf.file_refine(tmp_path / "reads.blow5", ref_txt, batch=4, raise_on_corrupt=False, **kw)
    assert fids == [ids[i] for i in keep] and flines["cost_refined"].tolist() == [int(want.rows[i]["cost"]) if want.rows[i]["qlen"] else -1 for i in keep]
    assert flines["fit"].tolist() == [names.get(int(want.status[i]), b"*") for i in keep]
    with pytest.raises(gpu.lib.S5GpuError):
        rf.file_refine(tmp_path / "reads.blow5", ref_txt, **kw)
    # --per-event: the lines of s5align from the refined path
    p = subprocess.run([rf.S5REFINE, "--per-event"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1
    lines = []
    for i in keep:
        ql = int(want.rows[i]["qlen"])
        if ql == 0:
            lines.append(ids[i] + b"\t*\t*\t*\t*\t*\t*\n")
        for k in range(ql):
            e = b_ev[i, k]
            lines.append(b"%s\t%d\t%d\t%d\t%s\t%d\t%d\n" % (ids[i], skip + k, e["start"], e["start"] + e["length"], b"%.6g" % float(e["mean"]), want.lo[i, k], want.hi[i, k]))
    assert p.stdout == b"".join(lines)
    # --iters 1 --slope: the parameters reach the call
    p = subprocess.run([rf.S5REFINE, "--iters", "1", "--slope", "0.001,0.002"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and [l.split(b"\t")[7] for l in p.stdout.splitlines() if b"*" not in l] == [b"0"] * 4
    assert subprocess.run([rf.S5REFINE], capture_output=True).returncode == 2
    for badarg in (["--iters", "5"], ["--pad", "65536"], ["--slope", "2,1"], ["--slope", "x"]):
        assert subprocess.run([rf.S5REFINE] + badarg + args, capture_output=True).returncode == 2, badarg
