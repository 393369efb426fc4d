"""map: subsequence DTW of each read's events against a reference squiggle on the device (docs/codecs.md §4.16;
slow5tools_amd/csrc/dtw_kernels.hip).

The oracle is the numpy restatement of §4.16 in dtw_ref.py: the quantiser in float64 summed strictly left to right, and sDTW with the
matrices D and S and the tie rule, vectorised over anti-diagonals (and over a batch of queries of one length).  The definition is integer
from the quantiser onward, so the device is held to it exactly on all four columns of a row.  The code a lane of k_sdtw runs (dtw_dev.h) is
plain C++: it is also compiled for the CPU, 64 lanes in a loop with the lane exchange passed in as a function, and held to the same oracle.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from blow5_fixture import Blow5, golden
from chain_common import DNA, EMPTY, EVENT, MAP_ROW, NO_COST, QUERY_SHORT, ROOT, host_build, levels_signal, record
from chain_common import gpu  # noqa: F401
from dtw_ref import QLENS, RS, _g_of, known_answer_cases, last_lane_batch, map_lines, quant_ref, rows_ref, sdtw_ref
from dtw_ref import map_ref, mixed_batches  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = ["s5gpu_quantise_host", "s5gpu_event_queries_dev", "s5gpu_sdtw_dev", "s5gpu_map_batch"]


def test_library_exports_the_map_calls():
    from slow5tools_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [5, 9, 9, 11]


def test_map_layouts_match_header(tmp_path):
    from slow5tools_amd import _lib
    from slow5tools_amd import map as smap

    row, pr = ["cost", "qlen", "start", "end"], ["skip", "qmax", "qmin", "scale", "clip", "want_start"]
    src = tmp_path / "ly.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){printf("%zu", sizeof(s5gpu_map_row_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_map_row_t, %s));\n' % m for m in row)
                   + 'printf(" %zu", sizeof(s5gpu_map_params_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_map_params_t, %s));\n' % m for m in pr)
                   + 'printf(" %d\\n", S5GPU_STATUS_QUERY_SHORT);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "ly")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ly")], text=True).split()]
    D, Pm = smap.MAP_ROW, _lib.MapParams
    assert got == [D.itemsize] + [D.fields[m][1] for m in row] + [C.sizeof(Pm)] + [getattr(Pm, m).offset for m in pr] + [_lib.STATUS_QUERY_SHORT]
    assert D.itemsize == 16 and D == MAP_ROW and _lib.STATUS_QUERY_SHORT == QUERY_SHORT


def test_s5map_exists_after_build():
    from slow5tools_amd import build
    from slow5tools_amd import map as smap

    build.build()
    assert os.access(smap.S5MAP, os.X_OK)


def _half_way_input():
    """64 values m with mean exactly 0 and standard deviation exactly 16, so that ((m - mu) / sd) * 32 = 2 m: the values k / 2 + 1 / 4 land
    exactly on k + 0.5.  Every value is a multiple of 1 / 4, so every sum and square below is exact in float64: 9 half-way values, 19 of
    16.0 and four more whose squares fill the sum of squares up to 64 * 256, each with its negative."""
    half = [0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.25, 10.25, 10.75]
    rest = int((64 * 256 - 2 * sum(h * h for h in half) - 38 * 256) * 16) // 2          # the sum of a^2 over the four values a / 4
    four = next((a, b, c, d) for a in range(int(rest ** 0.5), -1, -1) for b in range(a, -1, -1) if a * a + b * b <= rest
                for c in range(b, -1, -1) if a * a + b * b + c * c <= rest
                for d in [int(round((rest - a * a - b * b - c * c) ** 0.5))] if d <= c and a * a + b * b + c * c + d * d == rest)
    pos = half + [16.0] * 19 + [v / 4.0 for v in four]
    m = np.array(pos + [-v for v in pos], dtype=np.float32)
    assert len(m) == 64 and np.array_equal(m.astype(np.float64), np.array(pos + [-v for v in pos]))
    return m, half


def test_quantise_host_equals_the_restatement():
    from slow5tools_amd import map as smap

    rng = np.random.default_rng(1)
    cases = [np.zeros(0, np.float32), np.array([5.5], np.float32), np.full(40, 81.25, np.float32),
             np.array([0.0] * 99 + [1000.0], np.float32),                                      # one value far beyond the clip
             np.array([1.0, 2.0, np.nan, 4.0], np.float32), np.array([1.0, np.inf, 3.0], np.float32), np.array([-np.inf, 1.0, np.inf], np.float32),
             np.array([3e38, -3e38, 3e38, 3e38], np.float32),
             rng.normal(90.0, 12.0, 100000).astype(np.float32), (rng.normal(0.0, 1.0, 1000) * 1e-3).astype(np.float32)]
    for m in cases:
        for scale, clip in ((32.0, 127), (1000.0, 32767), (0.5, 1)):
            got = smap.quantise(m, scale, clip)
            assert got.dtype == np.int16 and np.array_equal(got, quant_ref(m, scale, clip)), (len(m), scale, clip)
    assert not smap.quantise(cases[2]).any() and not smap.quantise(cases[4]).any() and not smap.quantise(cases[5]).any()
    assert smap.quantise(cases[3])[-1] == 127 and smap.quantise(cases[8]).std() > 30
    # half-way points: mu = 0 and sd = 16 exactly, so ((m - mu) / sd) * 32 = 2 m = k + 0.5 exactly, and rint goes to the even neighbour
    m, half = _half_way_input()
    d = m.astype(np.float64)
    assert np.cumsum(d)[-1] == 0.0 and np.sqrt(np.cumsum(d * d)[-1] / 64.0) == 16.0
    got = smap.quantise(m)
    assert np.array_equal(got, quant_ref(m))
    want = [int(2 * h) + (int(2 * h) & 1) for h in half]                   # k + 0.5 -> the even one of k and k + 1
    assert got[:9].tolist() == want and got[32:41].tolist() == [-w for w in want] and want[:4] == [0, 2, 2, 4]
    # refused
    L = __import__("slow5tools_amd._lib", fromlist=["lib"]).lib()
    q = np.full(4, 77, dtype=np.int16)
    f = np.ones(4, dtype=np.float32)
    for scale, clip in ((0.0, 127), (-1.0, 127), (float("nan"), 127), (float("inf"), 127), (32.0, 0), (32.0, 32768), (32.0, -5)):
        assert L.s5gpu_quantise_host(f.ctypes.data_as(C.c_void_p), 4, scale, clip, q.ctypes.data_as(C.c_void_p)) == -1
    assert (q == 77).all()


LANES_HOST = r'''
// The code a lane of k_sdtw runs (dtw_dev.h) on the CPU: 64 lanes in a loop, in lockstep, the lane exchange passed in as a function.
// in.bin holds cases, out.bin gets two rows (without and with want_start) or the quantised values of each.
#define S5_DTW_HOST
#include "dtw_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace dtwk;
typedef void (*Shift)(const uint32_t *v, uint32_t fill, uint32_t *out);        // out[l] = v[l - 1], out[0] = fill: the wave shift
static void shift_up1(const uint32_t *v, uint32_t fill, uint32_t *out) { for (int l = 63; l >= 1; l--) out[l] = v[l - 1]; out[0] = fill; }

template <int G, bool WS, int KB>
static U4 run(const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R, Shift shift) {
    std::vector<Lane<G, WS> > L(64);
    uint32_t rcur[64], v[64], r[64], up[64], sup[64];
    for (uint32_t l = 0; l < 64; l++) {
        lane_init(L[l], l == 0);
        rcur[l] = 0; sup[l] = 0xFFFFFFFFu;
        for (int k = 0; k < G; k++) { const uint32_t row = l * G + k; L[l].q[k] = biased(row < Q ? q[row] : (int16_t)0); }
    }
    const uint32_t last = (Q - 1) / G, steps = R + last;
    if ((int)(Q - 1 - last * G) != KB) abort();
    for (uint32_t t = 0; t < steps; t++) {                                 // every lane steps at every step, as on the device
        const uint32_t r0 = biased(t < R ? ref[t] : (int16_t)0);
        shift(rcur, r0, r);
        for (int l = 0; l < 64; l++) { rcur[l] = r[l]; v[l] = L[l].d[G - 1]; }
        shift(v, 0u, up);
        if (WS) { for (int l = 0; l < 64; l++) v[l] = (uint32_t)L[l].s[G - 1]; shift(v, t + 1, sup); }
        for (uint32_t l = 0; l < 64; l++) {
            lane_step(L[l], r[l], up[l], (int32_t)sup[l]);
            lane_best<G, WS, KB>(L[l], t - l, R);
        }
    }
    return result_row(L[last].best, Q, WS ? L[last].best_start : -1, L[last].best_end);
}
template <int G, int KB = 0>
struct Pick {
    static void go(int kb, const int16_t *q, uint32_t Q, const int16_t *ref, uint32_t R, U4 *out) {
        if (kb == KB) { out[0] = run<G, false, KB>(q, Q, ref, R, shift_up1); out[1] = run<G, true, KB>(q, Q, ref, R, shift_up1); }
        else if constexpr (KB + 1 < G) Pick<G, KB + 1>::go(kb, q, Q, ref, R, out);
    }
};
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (argc != 3 || !f || !o) return 1;
    for (;;) {
        uint32_t kind;
        if (fread(&kind, 4, 1, f) != 1) break;
        if (kind == 1) {                                                   // sDTW: Q, R, G, q, r
            uint32_t Q, R, G;
            if (fread(&Q, 4, 1, f) != 1 || fread(&R, 4, 1, f) != 1 || fread(&G, 4, 1, f) != 1 || Q < 1 || Q > 64 * G || R < 1) return 1;
            std::vector<int16_t> q(Q), r(R);
            if (fread(q.data(), 2, Q, f) != Q || fread(r.data(), 2, R, f) != R) return 1;
            const int kb = (int)((Q - 1) % G);
            U4 out[2];
            memset(out, 0xEE, sizeof out);
            if (G == 1) Pick<1>::go(kb, q.data(), Q, r.data(), R, out);
            else if (G == 2) Pick<2>::go(kb, q.data(), Q, r.data(), R, out);
            else if (G == 4) Pick<4>::go(kb, q.data(), Q, r.data(), R, out);
            else if (G == 8) Pick<8>::go(kb, q.data(), Q, r.data(), R, out);
            else if (G == 16) Pick<16>::go(kb, q.data(), Q, r.data(), R, out);
            else return 1;
            fwrite(out, 16, 2, o);
        } else {                                                           // quant: L, stride, scale, clip, m[L * stride]
            uint32_t L, stride; double scale; int32_t clip;
            if (fread(&L, 4, 1, f) != 1 || fread(&stride, 4, 1, f) != 1 || fread(&scale, 8, 1, f) != 1 || fread(&clip, 4, 1, f) != 1) return 1;
            std::vector<float> m((size_t)L * stride + 1);
            std::vector<int16_t> q(L + 1);
            if (fread(m.data(), 4, (size_t)L * stride, f) != (size_t)L * stride) return 1;
            if (L) quant_row(m.data(), stride, L, scale, clip, q.data());
            fwrite(q.data(), 2, L, o);
        }
    }
    return fclose(o) == 0 ? 0 : 1;
}
'''


def test_the_lane_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """lane_init, lane_step, lane_best and the quantiser of dtw_dev.h as g++ compiles them, contraction off: Q on both sides of the lane
    boundaries, R below, at and above the 64 lanes; the lane height the kernel would take and a larger one; values of +-127, of {-1, 0, 1}
    (ties) and of the full int16 range with the cells of the largest query at their bound"""
    rng = np.random.default_rng(9)
    dtw = []
    for Q in (1, 63, 64, 65, 130):
        for R in (1, 64, 300):
            dtw.append((rng.integers(-127, 128, Q), rng.integers(-127, 128, R), _g_of(Q)))
            dtw.append((rng.integers(-1, 2, Q), rng.integers(-1, 2, R), _g_of(Q)))
    dtw.append((rng.integers(-127, 128, 5), rng.integers(-127, 128, 70), 4))            # a lane height above the smallest: most lanes idle
    dtw.append((rng.integers(-127, 128, 130), rng.integers(-127, 128, 64), 16))
    dtw.append((rng.integers(-32768, 32768, 257), rng.integers(-32768, 32768, 90), 8))
    dtw.append((rng.integers(-32768, 32768, 1000), rng.integers(-32768, 32768, 70), 16))
    dtw.append((np.full(1024, 32767), np.full(65, -32768), 16))                          # D[1023][j] = 65535 * 1024
    dtw = [(np.asarray(q, dtype=np.int16), np.asarray(r, dtype=np.int16), g) for q, r, g in dtw]
    quant = [(rng.normal(90, 12, L).astype(np.float32), stride, scale, clip)
             for L in (0, 1, 2, 50, 250, 1024) for stride, scale, clip in ((1, 32.0, 127), (4, 32.0, 127), (4, 3000.0, 32767))]
    quant.append((np.full(30, 4.5, np.float32), 4, 32.0, 127))
    quant.append((np.array([1.0, np.nan, 2.0, 3.0], np.float32), 1, 32.0, 127))
    quant.append((_half_way_input()[0], 1, 32.0, 127))
    with open(tmp_path / "in.bin", "wb") as fh:
        for q, r, g in dtw:
            fh.write(struct.pack("<IIII", 1, len(q), len(r), g) + q.tobytes() + r.tobytes())
        for m, stride, scale, clip in quant:
            wide = np.full((len(m), stride), 1e30, dtype=np.float32)       # what stands between the means must not matter
            wide[:, 0] = m
            fh.write(struct.pack("<IIIdi", 2, len(m), stride, scale, clip) + wide.tobytes())
    exe = host_build(tmp_path, "lanes_host", LANES_HOST, ["-O1", "-std=c++17", "-ffp-contract=off"])
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw, at = (tmp_path / "out.bin").read_bytes(), 0
    for q, r, g in dtw:
        got = np.frombuffer(raw, MAP_ROW, 2, at)
        at += 32
        c, s, e = sdtw_ref(q, r)
        assert got[0].tolist() == (c, len(q), -1, e) and got[1].tolist() == (c, len(q), s, e), (len(q), len(r), g)
    assert sdtw_ref(*dtw[-1][:2])[0] == 65535 * 1024
    for m, stride, scale, clip in quant:
        got = np.frombuffer(raw, np.int16, len(m), at)
        at += 2 * len(m)
        assert np.array_equal(got, quant_ref(m, scale, clip)), (len(m), stride, scale, clip)
    assert at == len(raw)


def test_restatement_on_hand_made_matrices():
    # one row: the cost is the nearest reference value, the first of equals
    assert sdtw_ref([5], [9, 4, 6, 4]) == (1, 1, 1)
    # the start is free, the end is not the last column
    assert sdtw_ref([1, 2, 3], [7, 7, 1, 2, 3, 7]) == (0, 2, 4)
    # a query longer than the reference walks down column by column
    assert sdtw_ref([1, 1, 1, 2, 2], [1, 2]) == (0, 0, 1)
    assert sdtw_ref([3, 3], [0]) == (6, 0, 0)
    # ties: all zeros, every cell 0; the smallest end, and from there the diagonal first, so start = end - (Q - 1) while it can
    assert sdtw_ref([0, 0, 0], [0, 0, 0, 0, 0]) == (0, 0, 0)
    c, s, e = sdtw_ref(np.zeros((2, 3)), [5, 0, 0, 0])
    assert c.tolist() == [0, 0] and e.tolist() == [1, 1] and s.tolist() == [1, 1]
    # the batch form equals the single form
    rng = np.random.default_rng(2)
    q, r = rng.integers(-3, 4, (6, 17)), rng.integers(-3, 4, 40)
    c, s, e = sdtw_ref(q, r)
    assert [sdtw_ref(q[b], r) for b in range(6)] == list(zip(c.tolist(), s.tolist(), e.tolist()))


def test_restatement_finds_the_known_span():
    """the warped slice [a, a + Q) of the reference aligns at cost 0 from a to a + Q - 1 (seed KNOWN_SEED; draws whose level sequence stands in
    the reference twice are dropped: at least 20 remain)"""
    ref, cases = known_answer_cases()
    assert len(cases) >= 20 and np.abs(np.diff(ref.astype(np.int64))).min() >= 20
    assert any(len(q) > Q for q, a, Q, _ in cases)
    for q, a, Q, _ in cases:
        assert sdtw_ref(q, ref) == (0, a, a + Q - 1), (a, Q)


# ---------------------------------------------------------------------------------------------------------------- gpu

def _run_sdtw(env, qm, qlens, ref, want_start, pitch=None):
    """s5gpu_sdtw_dev on a query matrix (numpy [n, pitch] int16) with guard rows around out_rows -> MAP_ROW array.  Guards and inputs are
    checked here."""
    torch, L = env.torch, env.L
    n = len(qlens)
    d_q = torch.from_numpy(np.ascontiguousarray(qm)).to("cuda")
    d_ql = torch.from_numpy(np.asarray(qlens, dtype=np.int32)).to("cuda")
    d_r = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16)).to("cuda")
    d_out = torch.full(((n + 2) * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    env.lib.check(L.s5gpu_sdtw_dev(n, d_q.data_ptr(), qm.shape[1] if pitch is None else pitch, d_ql.data_ptr(), d_r.data_ptr(), len(ref), int(want_start),
                                   d_out.data_ptr() + 16, None), "s5gpu_sdtw_dev")
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:4] == 0x5A5A5A5A).all() and (out[-4:] == 0x5A5A5A5A).all(), "a guard row around out_rows was written"
    assert np.array_equal(d_q.cpu().numpy(), qm) and np.array_equal(d_r.cpu().numpy(), np.asarray(ref, dtype=np.int16))
    return out[4:-4].view(MAP_ROW).copy()


def _check_rows(got, want, what):
    for col in ("cost", "qlen", "start", "end"):
        bad = np.nonzero(got[col] != want[col])[0]
        assert len(bad) == 0, (what, col, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("R", RS)
def test_sdtw_is_exact_on_a_mixed_batch(gpu, mixed_batches, R):
    rng = np.random.default_rng(100 + R)
    qm, ref = mixed_batches["pm127"], rng.integers(-127, 128, R).astype(np.int16)
    want = rows_ref(qm, QLENS, ref, True)
    assert want["cost"][0] == NO_COST and (want["cost"][1:] < 2 ** 26).all()
    for ws in (False, True):
        w = want.copy()
        if not ws:
            w["start"] = -1
        _check_rows(_run_sdtw(gpu, qm, QLENS, ref, ws), w, (R, ws))


@pytest.mark.gpu
def test_sdtw_every_row_of_the_last_lane(gpu):
    qm, ql = last_lane_batch()
    ref = np.random.default_rng(42).integers(-127, 128, 129).astype(np.int16)
    want = rows_ref(qm, ql, ref, True)
    assert want["qlen"].tolist() == ql and (want["cost"] < 2 ** 26).all() and (want["start"] >= 0).all()       # every read has a result
    for ws in (False, True):
        w = want.copy()
        if not ws:
            w["start"] = -1
        _check_rows(_run_sdtw(gpu, qm, ql, ref, ws), w, ("every row of the last lane", ws))


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 65, 129, 500])
def test_sdtw_ties_take_the_smallest_end_and_the_predecessor_order(gpu, mixed_batches, R):
    rng = np.random.default_rng(200 + R)
    qm, ref = mixed_batches["ties"], rng.integers(-1, 2, R).astype(np.int16)
    want = rows_ref(qm, QLENS, ref, True)
    _check_rows(_run_sdtw(gpu, qm, QLENS, ref, True), want, (R, True))
    want["start"] = -1
    _check_rows(_run_sdtw(gpu, qm, QLENS, ref, False), want, (R, False))


@pytest.mark.gpu
def test_sdtw_full_int16_range_at_the_overflow_bound(gpu):
    """Q = 1024 over the whole int16 range; against a reference of -32768 the query of 32767 has every cell of its last row at 65535 * 1024"""
    rng = np.random.default_rng(6)
    qm = np.zeros((3, 1024), dtype=np.int16)
    qm[0], qm[1], qm[2, :1000] = 32767, rng.integers(-32768, 32768, 1024), rng.integers(-32768, 32768, 1000)
    ql = [1024, 1024, 1000]
    for ref in (np.full(65, -32768, dtype=np.int16), rng.integers(-32768, 32768, 129).astype(np.int16)):
        want = rows_ref(qm, ql, ref, True)
        _check_rows(_run_sdtw(gpu, qm, ql, ref, True), want, len(ref))
    assert rows_ref(qm[:1], ql[:1], np.full(65, -32768, dtype=np.int16), True)[0].tolist() == (65535 * 1024, 1024, 0, 0)


@pytest.mark.gpu
def test_sdtw_many_waves_and_workgroups(gpu):
    rng = np.random.default_rng(8)
    qm, ref = rng.integers(-127, 128, (200, 64)).astype(np.int16), rng.integers(-127, 128, 129).astype(np.int16)
    c, s, e = sdtw_ref(qm, ref)
    want = np.zeros(200, dtype=MAP_ROW)
    want["cost"], want["qlen"], want["start"], want["end"] = c, 64, s, e
    _check_rows(_run_sdtw(gpu, qm, [64] * 200, ref, True), want, "n = 200")
    assert len(set(want["end"].tolist())) > 20
    # a pitch below the matrix's own: the queries are the first 40 values of every 64, qlen beyond the pitch is the pitch
    got = _run_sdtw(gpu, qm.reshape(320, 40), [40] * 319 + [64], ref, False, pitch=40)
    c, s, e = sdtw_ref(qm.reshape(320, 40), ref)
    assert np.array_equal(got["cost"], c) and np.array_equal(got["end"], e) and (got["qlen"] == 40).all() and (got["start"] == -1).all()


@pytest.mark.gpu
def test_sdtw_dev_finds_the_known_span(gpu):
    torch = gpu.torch
    ref, cases = known_answer_cases()
    pitch = max(len(q) for q, a, Q, _ in cases)
    qm = np.zeros((len(cases), pitch), dtype=np.int16)
    for i, (q, a, Q, _) in enumerate(cases):
        qm[i, :len(q)] = q
    ql = [len(q) for q, a, Q, _ in cases]
    out = gpu.map.sdtw_dev(torch.from_numpy(qm).to("cuda"), torch.from_numpy(np.array(ql, dtype=np.int32)).to("cuda"), torch.from_numpy(ref).to("cuda"),
                           want_start=True)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (len(cases), 4)
    got = out.cpu().numpy().view(MAP_ROW).reshape(-1)
    assert len(cases) >= 20
    assert got.tolist() == [(0, len(q), a, a + Q - 1) for q, a, Q, _ in cases]


@pytest.fixture(scope="module")
def decoded(gpu):
    """a decoded mixed batch with one record that fails to decode, and its event rows as the library makes them"""
    rng = np.random.default_rng(12)
    lengths = [0, 5, 70, 400, 4000, 20000, 400]
    recs = [record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
    bad = bytearray(recs[6])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[6] = bytes(bad)
    dec = gpu.press.decode_to_device(recs)
    f = dec.t_fields.cpu().numpy().view(gpu.lib.REC_FIELDS)[:len(recs)].copy()
    assert not f["status"][:6].any() and f["status"][6] != 0
    rows, first = gpu.events.events_dev(dec, DNA, "raw")
    env = type("Env", (), {})()
    env.dec, env.fields, env.rows, env.first, env.n = dec, f, rows, first, len(recs)
    env.h_rows, env.h_first = rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    counts = np.diff(env.h_first)
    assert counts[0] == 0 and counts[6] == 0 and counts[1] == 1 and counts[3] > 10 and counts[5] > 1000
    return env


def _queries_want(d, skip, qmax, qmin):
    qm, ql, st = np.zeros((d.n, qmax), dtype=np.int16), np.zeros(d.n, dtype=np.int32), np.zeros(d.n, dtype=np.int32)
    for i in range(d.n):
        ev = d.h_rows[d.h_first[i]:d.h_first[i + 1]]
        n = min(qmax, max(len(ev) - skip, 0))
        if d.fields["status"][i] != 0:
            n, st[i] = 0, d.fields["status"][i]
        elif n < qmin:
            n, st[i] = 0, QUERY_SHORT
        ql[i] = n
        qm[i, :n] = quant_ref(ev["mean"][skip:skip + n])
    return qm, ql, st


@pytest.mark.gpu
@pytest.mark.parametrize("skip,qmax,qmin", [(0, 1, 1), (0, 64, 10), (3, 64, 64), (0, 250, 30), (3, 250, 250), (3, 1, 1)])
def test_event_queries_are_the_quantised_means(gpu, decoded, skip, qmax, qmin):
    torch, d = gpu.torch, decoded
    fst = torch.from_numpy(d.fields["status"].astype(np.int32)).to("cuda")
    q, ql, st = gpu.map.queries_dev(d.rows, d.first, fst, skip=skip, qmax=qmax, qmin=qmin)
    assert q.is_cuda and q.dtype == torch.int16 and tuple(q.shape) == (d.n, qmax)
    wq, wl, ws = _queries_want(d, skip, qmax, qmin)
    assert ql.cpu().numpy().tolist() == wl.tolist() and st.cpu().numpy().tolist() == ws.tolist()
    assert np.array_equal(q.cpu().numpy(), wq)
    assert ws[6] == d.fields["status"][6] != QUERY_SHORT and ws[0] == QUERY_SHORT and wl[5] == qmax
    if qmin > 1:
        assert (ws[:6] == QUERY_SHORT).sum() >= 2 and (ws[:6] == 0).sum() >= 2
    if qmax > 1:
        assert np.abs(wq[5].astype(np.int64)).max() > 20 and abs(int(wq[5].astype(np.int64).sum())) < 16 * qmax


def _map_want(gpu, dec, n, ref, skip, qmax, qmin, want_start):
    """events_dev + quant_ref + sdtw_ref on the host"""
    rows, first = gpu.events.events_dev(dec, DNA, "raw")
    h, fi = rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    f = dec.t_fields.cpu().numpy().view(gpu.lib.REC_FIELDS)[:n]
    want, st = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=np.int32)
    for i in range(n):
        ev = h[fi[i]:fi[i + 1]]
        m = min(qmax, max(len(ev) - skip, 0))
        if f["status"][i] != 0 or m < qmin:
            want[i], st[i] = EMPTY, (f["status"][i] if f["status"][i] != 0 else QUERY_SHORT)
            continue
        c, s, e = sdtw_ref(quant_ref(ev["mean"][skip:skip + m]), ref)
        want[i] = (c, m, s if want_start else -1, e)
    return want, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["exp_1_lossless.blow5", "gridr10dna_b3.blow5"])
def test_map_dev_and_read_map_on_golden_files(gpu, map_ref, name):
    f = Blow5(golden(name))
    n = len(f.records)
    dec = gpu.press.decode_to_device(f.records, f.rec_method, f.sig_method, no_payload=gpu.press.no_payload_methods(f.rec_method, f.sig_method))
    assert gpu.map.quantise(np.arange(5, dtype=np.float32)).tolist() == quant_ref(np.arange(5, dtype=np.float32)).tolist()
    for skip, qmax, qmin, ws in ((0, 250, 50, True), (5, 100, 100, False)):
        want, wst = _map_want(gpu, dec, n, map_ref, skip, qmax, qmin, ws)
        assert (want["qlen"] == qmax).all() and (want["cost"] > 0).all()
        got, st = gpu.map.map_dev(dec, map_ref, skip=skip, qmax=qmax, qmin=qmin, want_start=ws)
        assert got.dtype == MAP_ROW and got.tolist() == want.tolist() and st.tolist() == wst.tolist(), (name, "map_dev", skip, qmax)
        got, st = gpu.map.read_map(f.records, map_ref, f.rec_method, f.sig_method, skip=skip, qmax=qmax, qmin=qmin, want_start=ws)
        assert got.dtype == MAP_ROW and got.tolist() == want.tolist() and st.tolist() == wst.tolist(), (name, "read_map", skip, qmax)
    # a query no read is long enough for: every row empty, every status 18
    got, st = gpu.map.read_map(f.records, map_ref, f.rec_method, f.sig_method, skip=1 << 30, qmax=10, qmin=1)
    assert got.tolist() == [EMPTY] * n and st.tolist() == [QUERY_SHORT] * n


@pytest.mark.gpu
def test_map_batch_with_a_corrupt_record(gpu, map_ref):
    m = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    recs = list(m.records)
    good, st0 = gpu.map.read_map(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True)
    assert not st0.any() and (good["qlen"] == 64).all()
    bad = bytearray(recs[1])
    bad[-1] ^= 0x5A
    recs[1] = bytes(bad)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        gpu.map.read_map(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True)
    got, st = gpu.map.read_map(recs, map_ref, m.rec_method, m.sig_method, qmax=64, qmin=10, want_start=True, raise_on_error=False)
    assert st[1] not in (0, QUERY_SHORT) and not st[0] and not st[2:].any()
    assert got[1].tolist() == EMPTY and got[0] == good[0] and np.array_equal(got[2:], good[2:])


@pytest.mark.gpu
def test_s5map_prints_the_restatements_lines(gpu, tmp_path):
    rng = np.random.default_rng(31)
    levels = rng.normal(90.0, 12.0, 800).astype(np.float32)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n\n" + "".join("%.9g\n" % v for v in levels))
    ref = quant_ref(levels)
    m = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    n = len(m.records)
    dec = gpu.press.decode_to_device(m.records, m.rec_method, m.sig_method)
    ids = [g["read_id"] for g in gpu.press.decode_records(m.records, m.rec_method, m.sig_method)]
    counts = np.diff(gpu.events.events_dev(dec, DNA, "raw")[1].cpu().numpy())
    some = int(np.sort(counts)[n // 2])                                    # a query length that some reads reach and others do not
    for args, skip, qmax, qmin, ws in (([], 0, 250, 50, False), (["--start", "--events", "64", "--min-events", "20", "--skip", "2", "-K", "3"], 2, 64, 20, True),
                                       (["--start", "--events", str(some), "--min-events", str(some)], 0, some, some, True)):
        want, wst = _map_want(gpu, dec, n, ref, skip, qmax, qmin, ws)
        p = subprocess.run([gpu.map.S5MAP] + args + [str(ref_txt), golden("example_multi_rg_v0.2.0.blow5")], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout == map_lines(ids, want, ws), args
    assert 0 < (want["qlen"] == 0).sum() < n                               # the last run printed both kinds of line
    got_ids, got = gpu.map.file_map(golden("example_multi_rg_v0.2.0.blow5"), ref_txt, qmax=some, qmin=some, want_start=True)
    assert got_ids == ids and got.tolist() == want.tolist()
    # a corrupt record between good ones: its id on stderr, exit 1, the others printed
    raw = bytearray(m.raw)
    raw[m.offsets[1] + 8 + len(m.records[1]) - 1] ^= 0x5A
    (tmp_path / "bad.blow5").write_bytes(bytes(raw))
    want, wst = _map_want(gpu, dec, n, ref, 0, 64, 20, False)
    p = subprocess.run([gpu.map.S5MAP, "--events", "64", "--min-events", "20", str(ref_txt), str(tmp_path / "bad.blow5")], capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[1] in p.stderr
    keep = [i for i in range(n) if i != 1]
    assert p.stdout == map_lines([ids[i] for i in keep], want[keep], False)
    # an empty reference, an unparsable one, no arguments: exit 2
    (tmp_path / "empty.txt").write_text("# nothing\n\n")
    (tmp_path / "words.txt").write_text("1.5\nabc\n")
    for r in ("empty.txt", "words.txt", "missing.txt"):
        p = subprocess.run([gpu.map.S5MAP, str(tmp_path / r), golden("example_multi_rg_v0.2.0.blow5")], capture_output=True, timeout=120)
        assert p.returncode == 2 and p.stdout == b"", r
    assert subprocess.run([gpu.map.S5MAP], capture_output=True).returncode == 2
    assert subprocess.run([gpu.map.S5MAP, "--events", "2000", str(ref_txt), golden("example_multi_rg_v0.2.0.blow5")], capture_output=True).returncode == 2


@pytest.mark.gpu
def test_refused_arguments_write_nothing(gpu, decoded):
    torch, L, lib, d = gpu.torch, gpu.L, gpu.lib, decoded
    vp = C.c_void_p
    n = d.n
    d_q = torch.full((n, 64), 77, dtype=torch.int16, device="cuda")
    d_ql = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    d_st = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_out = torch.full((n * 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_ref = torch.zeros(100, dtype=torch.int16, device="cuda")
    fst = torch.from_numpy(d.fields["status"].astype(np.int32)).to("cuda")
    rows = d.rows.contiguous()

    def queries(pr, p_null=False, first=True):
        p = lib.MapParams(*pr)
        return L.s5gpu_event_queries_dev(n, rows.data_ptr(), d.first.data_ptr() if first else None, fst.data_ptr(), None if p_null else C.byref(p),
                                         d_q.data_ptr(), d_ql.data_ptr(), d_st.data_ptr(), None)
    nan, inf = float("nan"), float("inf")
    refused = [(0, 0, 1, 32.0, 127, 0), (0, 1025, 1, 32.0, 127, 0), (0, 64, 0, 32.0, 127, 0), (0, 64, 65, 32.0, 127, 0), (0, 64, 10, nan, 127, 0),
               (0, 64, 10, inf, 127, 0), (0, 64, 10, 0.0, 127, 0), (0, 64, 10, -32.0, 127, 0), (0, 64, 10, 32.0, 0, 0), (0, 64, 10, 32.0, 32768, 0)]
    ok = (0, 64, 10, 32.0, 127, 0)
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (vp * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    h_ref = np.zeros(100, dtype=np.int16)
    h_rows = np.full(1, 0xA5, dtype=np.uint8).repeat(16)
    h_st = np.full(1, -7, dtype=np.int32)

    def batch(pr, ev=DNA, R=100, ref=True, ev_null=False, mp_null=False):
        e, p = lib.EventParams(*ev), lib.MapParams(*pr)
        return L.s5gpu_map_batch(1, rec_p, rl, 1, 1, None if ev_null else C.byref(e), None if mp_null else C.byref(p),
                                 h_ref.ctypes.data_as(vp) if ref else None, R, h_rows.ctypes.data_as(vp), h_st.ctypes.data_as(vp))
    for pr in refused:
        assert queries(pr) == -1, pr
        assert batch(pr) == -1, pr
    assert queries(ok, p_null=True) == -1 and queries(ok, first=False) == -1
    assert batch(ok, R=0) == -1 and batch(ok, ref=False) == -1 and batch(ok, ev_null=True) == -1 and batch(ok, mp_null=True) == -1
    assert batch(ok, ev=(3, 3, 1.4, 9.0, 0.2)) == -1 and batch(ok, ev=(3, 6, nan, 9.0, 0.2)) == -1

    def sdtw(pitch=64, R=100, ref=True, q=True, out_off=0):
        return L.s5gpu_sdtw_dev(n, d_q.data_ptr() if q else None, pitch, d_ql.data_ptr(), d_ref.data_ptr() if ref else None, R, 1,
                                d_out.data_ptr() + out_off, None)
    assert sdtw(pitch=0) == -1 and sdtw(pitch=1025) == -1 and sdtw(R=0) == -1 and sdtw(R=1 << 31) == -1 and sdtw(ref=False) == -1 and sdtw(q=False) == -1
    assert sdtw(out_off=4) == -1
    torch.cuda.synchronize()
    assert (d_q.cpu().numpy() == 77).all() and (d_ql.cpu().numpy() == 7).all() and (d_st.cpu().numpy() == -7).all()      # nothing was launched
    assert (d_out.cpu().numpy() == 0x5A5A5A5A).all() and (h_rows == 0xA5).all() and (h_st == -7).all()
    assert queries(ok) == 0 and sdtw() == 0
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() != -7).all() and (d_out.cpu().numpy().view(MAP_ROW)["qlen"] == d_ql.cpu().numpy()).all()
