"""pileup: per-reference-position statistics of aligned events, accumulated on the device (docs/codecs.md §4.18;
slow5tools_amd/csrc/pileup_kernels.hip).

The oracle is pileup_ref of pileup_ref.py: the definition of §4.18 in int64 numpy, read by read, with the invariants asserted.  Every member of
the table is an integer sum, minimum or maximum, so the device is held to it byte for byte, whatever the window, the grid, the batches and
the streams.  Paths for the kernel tests are random valid monotone paths, not DTW's: the kernel only sees lo and hi.  The header's
validation, row accumulation, window and flush (pileup_dev.h) are plain C++: they are also compiled for the CPU and held to the same oracle.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from chain_common import BEHIND, DEFAULT_COLS, DEFAULT_GRID, DNA, EVENT, MAP_ROW, PATH_ROW, PATH_WIDE, PILE_COL, PILE_TOTAL, QUERY_SHORT, ROOT
from chain_common import Acc, host_build, levels_signal, pile_accum, pile_lines, record, synth_file
from chain_common import gpu  # noqa: F401
from dtw_ref import known_answer_cases, quant_ref
from pileup_ref import Case, _explain, flawed_cases, kernel_cases, mixed_case, pileup_ref, pitch40_case, same_columns_case, sums_case, table_bytes, window_case

# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = ["s5gpu_pileup_bytes", "s5gpu_pileup_reset_dev", "s5gpu_pileup_accum_dev", "s5gpu_pileup_open", "s5gpu_pileup_add_batch", "s5gpu_pileup_close"]


def test_library_exports_the_pileup_calls_and_the_tool_is_built(tmp_path):
    from slow5tools_amd import _lib, build, pileup

    build.build()
    assert os.access(pileup.S5PILEUP, os.X_OK)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [1, 3, 12, 5, 8, 2]
    assert _lib.PileCol == PILE_COL and _lib.PileCol.itemsize == 48 and pileup.PILE_COL == PILE_COL and pileup.PILE_TOTAL == PILE_TOTAL
    # a C program that uses the calls and the structs compiles against the header alone
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   'size_t (*a)(uint32_t) = s5gpu_pileup_bytes;\n'
                   'int (*b)(void *, uint32_t, void *) = s5gpu_pileup_reset_dev;\n'
                   'int (*c)(uint32_t, const int16_t *, uint32_t, const uint32_t *, const int16_t *, uint32_t, const int32_t *, const int32_t *, const int32_t *,'
                   ' const s5gpu_event_t *, void *, void *) = s5gpu_pileup_accum_dev;\n'
                   'void *(*d)(const s5gpu_event_params_t *, const s5gpu_map_params_t *, uint32_t, const int16_t *, uint32_t) = s5gpu_pileup_open;\n'
                   'int (*e)(void *, uint32_t, const void *const *, const size_t *, int, int, s5gpu_map_row_t *, int32_t *) = s5gpu_pileup_add_batch;\n'
                   'int (*f)(void *, void *) = s5gpu_pileup_close;\n'
                   'printf("%zu %zu %zu %zu %zu %d\\n", sizeof(s5gpu_pile_col_t), sizeof(s5gpu_pile_total_t), offsetof(s5gpu_pile_col_t, sum_q),'
                   ' offsetof(s5gpu_pile_col_t, min_q), offsetof(s5gpu_pile_total_t, R), a && b && c && d && e && f);return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == ["48", "64", "16", "40", "40", "1"]


def test_pileup_bytes():
    from slow5tools_amd import _lib

    f = _lib.lib().s5gpu_pileup_bytes
    for R in (1, 2, 65, 5000, 1 << 20, 1 << 26):
        assert f(R) == 64 + 48 * R, R
    assert f(0) == 0 and f((1 << 26) + 1) == 0 and f(0xFFFFFFFF) == 0


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) of the two device-pointer calls (the pointers are never dereferenced on the host, so made-up aligned addresses
    serve) and every refusal of open, which reads nothing but its parameters"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    P = 1 << 20                                                            # an aligned address

    def accum(n=4, q=P, pitch=64, ql=P, ref=P, R=100, lo=P, hi=P, st=P, ev=P, acc=P):
        return L.s5gpu_pileup_accum_dev(n, q, pitch, ql, ref, R, lo, hi, st, ev, acc, None)
    assert accum(pitch=0) == -1 and accum(pitch=1025) == -1 and accum(R=0) == -1 and accum(R=(1 << 26) + 1) == -1 and accum(R=1 << 31) == -1
    for name in ("q", "ql", "ref", "lo", "hi", "st", "acc"):
        assert accum(**{name: None}) == -1, name
    assert accum(q=P + 1) == -1 and accum(ql=P + 2) == -1 and accum(ref=P + 1) == -1 and accum(lo=P + 2) == -1 and accum(hi=P + 1) == -1
    assert accum(st=P + 2) == -1 and accum(ev=P + 8) == -1 and accum(acc=P + 8) == -1
    assert accum(n=0) == 0 and accum(n=0, ev=None, q=None, lo=None) == 0   # nothing to do: nothing is launched
    assert accum(n=0, acc=None) == -1 and accum(n=0, R=0) == -1
    assert L.s5gpu_pileup_reset_dev(None, 100, None) == -1 and L.s5gpu_pileup_reset_dev(P + 8, 100, None) == -1
    assert L.s5gpu_pileup_reset_dev(P, 0, None) == -1 and L.s5gpu_pileup_reset_dev(P, (1 << 26) + 1, None) == -1
    # open: NULL and a reason that names the argument, before a device is asked for
    vp = C.c_void_p
    h_ref = np.zeros(100, dtype=np.int16)

    def opened(pr=(0, 64, 10, 32.0, 127, 1), ev=DNA, wmax=256, R=100, ref=True, ev_null=False, mp_null=False):
        e, p = _lib.EventParams(*ev), _lib.MapParams(*pr)
        h = L.s5gpu_pileup_open(None if ev_null else C.byref(e), None if mp_null else C.byref(p), wmax, h_ref.ctypes.data_as(vp) if ref else None, R)
        return h, L.s5gpu_last_error()
    nan = float("nan")
    for pr in ((0, 0, 1, 32.0, 127, 1), (0, 1025, 1, 32.0, 127, 1), (0, 64, 0, 32.0, 127, 1), (0, 64, 65, 32.0, 127, 1), (0, 64, 10, nan, 127, 1),
               (0, 64, 10, 0.0, 127, 1), (0, 64, 10, 32.0, 0, 1), (0, 64, 10, 32.0, 32768, 1)):
        h, why = opened(pr=pr)
        assert h is None and why.startswith(b"s5gpu_pileup_open:") and b"device" not in why, (pr, why)
    for kw, word in ((dict(wmax=0), b"wmax"), (dict(wmax=(1 << 20) + 1), b"wmax"), (dict(R=0), b"reference"), (dict(R=(1 << 26) + 1), b"columns"),
                     (dict(ref=False), b"NULL"), (dict(mp_null=True), b"NULL"), (dict(pr=(0, 1024, 10, 32.0, 127, 1), wmax=1 << 20), b"scratch")):
        h, why = opened(**kw)
        assert h is None and word in why and b"device" not in why, (kw, why)
    assert opened(ev_null=True)[0] is None and opened(ev=(3, 3, 1.4, 9.0, 0.2))[0] is None
    assert L.s5gpu_pileup_add_batch(None, 0, None, None, 1, 1, None, None) == -1 and L.s5gpu_pileup_close(None, None) == 0


def test_the_options_refuse_bad_values():
    from slow5tools_amd import _lib

    L = _lib.lib()
    for key, bad, good in ((b"pileup_lds_cols", (-1, 1, 32, 63, 65, 96, 1000, 2048), (0, 64, 128, 256, 512, 1024, DEFAULT_COLS)),
                           (b"pileup_grid", (0, -1, 1025), (1, 7, 1024, DEFAULT_GRID))):
        for v in bad:
            assert L.s5gpu_set_option(key, v) == -1, (key, v)
        for v in good:                                                     # (the defaults last)
            assert L.s5gpu_set_option(key, v) == 0, (key, v)


PILE_HOST = r'''
// The code of k_pileup that lives in pileup_dev.h, on the CPU, with plain adds in place of the atomics: every read validated row by row, then
// its rows' cells added to the window's table (exactly `cols` columns at `wlo`) or to the table (exactly R columns), the window flushed at
// the end.  in.bin: n, pitch, R, events?, cols, wlo, then qlen, status, queries, ref, lo, hi, events; out.bin: the accumulator's bytes.
#define S5_PILEUP_HOST
#include "pileup_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace pilek;
struct HostOps {
    static void add64(uint64_t *p, uint64_t v) { *p += v; }
    static void minmax32(s5gpu_pile_col_t *c, int32_t lo, int32_t hi) { if (lo < c->min_q) c->min_q = lo; if (hi > c->max_q) c->max_q = hi; }
};
static s5gpu_pile_col_t *empty_cols(size_t k) {
    s5gpu_pile_col_t *c = (s5gpu_pile_col_t *)malloc(k ? k * sizeof *c : 1);
    if (!c) abort();
    for (size_t x = 0; x < k; x++) { memset(&c[x], 0, sizeof c[x]); c[x].min_q = 32767; c[x].max_q = -32768; }
    return c;
}
template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t k) { v.resize(k); return k == 0 || fread(v.data(), sizeof(T), k, f) == k; }

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t h[6];
    if (!f || !o || fread(h, 4, 6, f) != 6) return 1;
    const uint32_t n = h[0], pitch = h[1], R = h[2], cols = h[4];
    std::vector<uint32_t> qlen;
    std::vector<int32_t> status, lo, hi;
    std::vector<int16_t> q, ref;
    std::vector<s5gpu_event_t> ev;
    const size_t cells_in = (size_t)n * pitch;
    if (!get(f, qlen, n) || !get(f, status, n) || !get(f, q, cells_in) || !get(f, ref, R) || !get(f, lo, cells_in) || !get(f, hi, cells_in) ||
        !get(f, ev, h[3] ? cells_in : 0))
        return 1;
    s5gpu_pile_col_t *table = empty_cols(R), *win = empty_cols(cols);
    Window W;
    W.lo = h[5]; W.cols = cols;
    s5gpu_pile_total_t T;
    memset(&T, 0, sizeof T);
    T.R = R;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t Q = rows_of(qlen[k], pitch);
        if (status[k] != 0 || Q == 0) { T.reads_skipped++; continue; }
        const int32_t *l = lo.data() + (size_t)k * pitch, *u = hi.data() + (size_t)k * pitch;
        bool ok = true;
        for (uint32_t i = 0; i < Q; i++) ok = ok && row_ok(i, l[i], u[i], i ? u[i - 1] : 0, R);
        if (!ok) { T.reads_bad++; continue; }
        T.reads_used++;
        for (uint32_t i = 0; i < Q; i++)
            row_cells<HostOps>(i, l[i], u[i], i ? u[i - 1] : 0, (int32_t)q[(size_t)k * pitch + i], h[3] ? ev[(size_t)k * pitch + i].length : 0u, ref.data(), R, W,
                               win, table, &T.cells, &T.cost);
    }
    for (uint32_t b = 0; b < cols; b++) {
        const uint32_t j = W.lo + b;
        if (j >= W.lo && j < R) col_merge<HostOps>(table + j, win + b);
        else if (win[b].n_events) return 2;                                // a cell went to a slot that stands for no column
    }
    fwrite(&T, sizeof T, 1, o);
    fwrite(table, sizeof *table, R, o);
    free(table); free(win);
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _build_pile_host(tmp_path, extra=()):
    return host_build(tmp_path, "pile_host", PILE_HOST, ["-O1", "-std=c++17", "-Wall"], extra)


def _anchor(case):
    """where k_pileup's first workgroup puts its window: the smallest valid lo[0] of the first four reads"""
    at = [int(case.lo[k, 0]) for k in range(min(4, case.n)) if case.status[k] == 0 and min(int(case.qlen[k]), case.pitch) and 0 <= case.lo[k, 0] < case.R]
    return min(at) if at else 0


def _run_pile_host(exe, tmp_path, case, events, cols, wlo):
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<6I", case.n, case.pitch, case.R, int(events), cols, wlo))
        for a in (case.qlen, case.status, case.qm, case.ref, case.lo, case.hi) + ((case.ev,) if events else ()):
            fh.write(a.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return (tmp_path / "out.bin").read_bytes()


def run_header_on_the_cpu(tmp_path, extra=()):
    exe = _build_pile_host(tmp_path, extra)
    for name, case in kernel_cases().items():
        for events in (True, False):
            want = table_bytes(pileup_ref(case, events))
            plain = _run_pile_host(exe, tmp_path, case, events, 0, 0)
            assert plain == want, (name, events, _explain(plain, want))
            for wlo in {_anchor(case), 0, max(case.R - 10, 0)}:            # (the last: a window that hangs over the table's end)
                win = _run_pile_host(exe, tmp_path, case, events, 64, wlo)
                assert win == plain, (name, events, wlo, _explain(win, plain))


def test_restatement_on_hand_made_paths():
    # two reads on a reference of 6: read 0 rows (0..1), (1..1), (2..4); read 1 rows (1..1), (2..2)
    qm = np.array([[10, 20, 30], [5, -5, 0]], dtype=np.int16)
    lo, hi = np.array([[0, 1, 2], [1, 2, BEHIND]], dtype=np.int32), np.array([[1, 1, 4], [1, 2, BEHIND]], dtype=np.int32)
    ev = np.zeros((2, 3), dtype=EVENT)
    ev["length"] = [[4, 5, 6], [7, 8, 9]]
    total, cols = pileup_ref(Case(qm, [3, 2], [1, 2, 3, 4, 5, 6], lo, hi, ev=ev))
    assert cols["depth"].tolist() == [1, 2, 2, 1, 1, 0] and cols["n_events"].tolist() == [1, 3, 2, 1, 1, 0]
    assert cols["n_samples"].tolist() == [4, 4 + 5 + 7, 6 + 8, 6, 6, 0] and cols["sum_q"].tolist() == [10, 35, 25, 30, 30, 0]
    assert cols["sumsq_q"].tolist() == [100, 100 + 400 + 25, 900 + 25, 900, 900, 0] and cols["sum_cost"].tolist() == [9, 8 + 18 + 3, 27 + 8, 26, 25, 0]
    assert cols["min_q"].tolist() == [10, 5, -5, 30, 30, 32767] and cols["max_q"].tolist() == [10, 20, 30, 30, 30, -32768]
    assert tuple(total)[:6] == (2, 0, 0, 8, 124, 6)
    # the flawed reads are classified as §4.18 says, and the case makers make what they promise
    for name, (c, skipped, bad) in flawed_cases().items():
        t, _ = pileup_ref(c)
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (12 - skipped - bad, skipped, bad), name
    t, cols = pileup_ref(sums_case())
    assert cols["sumsq_q"][0] == 64 * 1024 * 32767 ** 2 > 2 ** 45 and cols["sum_cost"][0] == 64 * 1024 * 65535 and cols["depth"][0] == 64
    t, cols = pileup_ref(same_columns_case())
    assert np.flatnonzero(cols["n_events"]).min() >= 100 and np.flatnonzero(cols["n_events"]).max() == 129
    window_case()


def test_the_header_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """row_ok, row_cells, window_slot and col_merge of pileup_dev.h as g++ compiles them, over the cases of the GPU tests, with and without
    events, without a window and with one of 64 columns at the kernel's anchor, at column 0 and hanging over the table's end"""
    run_header_on_the_cpu(tmp_path)


# ---------------------------------------------------------------------------------------------------------------- gpu

def _options(env, cols=DEFAULT_COLS, grid=DEFAULT_GRID):
    env.lib.check(env.L.s5gpu_set_option(b"pileup_lds_cols", cols), "pileup_lds_cols")
    env.lib.check(env.L.s5gpu_set_option(b"pileup_grid", grid), "pileup_grid")


def _table(env, case, events=True, cols=DEFAULT_COLS, grid=DEFAULT_GRID):
    _options(env, cols, grid)
    try:
        return pile_accum(env, Acc(env, case.R), case, events)
    finally:
        _options(env)


@pytest.fixture(scope="module")
def wanted():
    """the restatement of a case, computed once: wanted(name, case, events) -> bytes"""
    memo = {}

    def get(name, case, events=True):
        if (name, events) not in memo:
            memo[name, events] = table_bytes(pileup_ref(case, events))
        return memo[name, events]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 200])
@pytest.mark.parametrize("R", [1, 65, 129, 5000])
def test_pileup_is_exact_on_a_mixed_batch(gpu, wanted, R, n):
    case = mixed_case(R, n)
    for events in (True, False):
        want = wanted(("mixed", R, n), case, events)
        for cols in (0, 64, DEFAULT_COLS):
            for grid in (1, DEFAULT_GRID):
                got = _table(gpu, case, events, cols, grid)
                assert got == want, (events, cols, grid, _explain(got, want))
    total = np.frombuffer(want[:64], PILE_TOTAL)[0]
    assert total["reads_skipped"] == sum(q == 0 for q in case.qlen) and total["reads_bad"] == 0 and total["R"] == R


@pytest.mark.gpu
def test_pileup_with_a_pitch_below_a_qlen(gpu, wanted):
    case = pitch40_case()
    for events in (True, False):
        for cols, grid in ((0, DEFAULT_GRID), (64, 1), (DEFAULT_COLS, DEFAULT_GRID)):
            got, want = _table(gpu, case, events, cols, grid), wanted("pitch 40", case, events)
            assert got == want, (events, cols, grid, _explain(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window edges", "same 30 columns"])
def test_pileup_window_edges(gpu, wanted, name):
    case = {"window edges": window_case, "same 30 columns": same_columns_case}[name]()
    want = wanted(name, case)
    for cols, grid in ((64, 1), (64, 2), (64, DEFAULT_GRID), (128, 1), (DEFAULT_COLS, 1), (DEFAULT_COLS, DEFAULT_GRID), (0, 1), (0, DEFAULT_GRID)):
        got = _table(gpu, case, True, cols, grid)
        assert got == want, (cols, grid, _explain(got, want))


@pytest.mark.gpu
def test_pileup_sums_are_64_bit(gpu, wanted):
    case = sums_case()
    want = wanted("sums", case)
    col0 = np.frombuffer(want[64:], PILE_COL)[0]
    assert col0["sumsq_q"] == 64 * 1024 * 32767 ** 2 and col0["sum_cost"] == 64 * 1024 * 65535 and col0["n_events"] == 65536
    for cols, grid in ((0, DEFAULT_GRID), (DEFAULT_COLS, DEFAULT_GRID), (64, 1)):
        got = _table(gpu, case, True, cols, grid)
        assert got == want, (cols, grid, _explain(got, want))


@pytest.mark.gpu
def test_pileup_leaves_out_skipped_and_bad_reads(gpu):
    for name, (case, skipped, bad) in flawed_cases().items():
        want = table_bytes(pileup_ref(case))
        for cols in (0, DEFAULT_COLS):
            got = _table(gpu, case, True, cols)
            assert got == want, (name, cols, _explain(got, want))
        t = np.frombuffer(got[:64], PILE_TOTAL)[0]
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (12 - skipped - bad, skipped, bad), name


@pytest.mark.gpu
def test_pileup_accumulates_over_calls_and_streams(gpu, wanted):
    torch = gpu.torch
    case = mixed_case(129, 200)
    want = wanted(("mixed", 129, 200), case)
    a, b = case.part(0, 90), case.part(90, 200)
    acc = Acc(gpu, case.R)
    empty = acc.bytes()
    assert empty == table_bytes(pileup_ref(case.part(0, 0)))               # what reset writes
    pile_accum(gpu, acc, a)
    got = pile_accum(gpu, acc, b)
    assert got == want, _explain(got, want)
    # the halves on two streams at once
    acc.reset()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    checks = [pile_accum(gpu, acc, a, stream=s1, sync=False), pile_accum(gpu, acc, b, stream=s2, sync=False)]
    torch.cuda.synchronize()
    got = [c() for c in checks][-1]
    assert got == want, _explain(got, want)
    acc.reset()
    assert acc.bytes() == empty


@pytest.mark.gpu
def test_pileup_after_the_real_chain(gpu):
    """the warped slices of dtw_ref.py through sdtw_dev, path_dev and accum_dev: every cost 0, depth the slices over a column, n_events the
    times their level was held"""
    torch, pl = gpu.torch, gpu.pileup
    ref, cases = known_answer_cases()
    assert len(cases) >= 20
    pitch = max(len(q) for q, a, Q, rep in cases)
    qm = np.zeros((len(cases), pitch), dtype=np.int16)
    for i, (q, a, Q, rep) in enumerate(cases):
        qm[i, :len(q)] = q
    ql = np.array([len(q) for q, a, Q, rep in cases], dtype=np.int32)
    d_q, d_ql, d_r = torch.from_numpy(qm).to("cuda"), torch.from_numpy(ql).to("cuda"), torch.from_numpy(ref).to("cuda")
    rows = gpu.map.sdtw_dev(d_q, d_ql, d_r, want_start=True)
    lo, hi, st = gpu.align.path_dev(d_q, d_ql, d_r, rows)
    acc = pl.new_acc(len(ref))
    assert acc.is_cuda and acc.dtype == torch.uint8 and acc.numel() == 64 + 48 * len(ref)
    assert pl.accum_dev(d_q, d_ql, d_r, lo, hi, st, acc) is acc
    total, cols = pl.to_host(acc)
    assert total.dtype == PILE_TOTAL and cols.dtype == PILE_COL and len(cols) == len(ref)
    depth, n_events = np.zeros(len(ref), np.int64), np.zeros(len(ref), np.int64)
    for q, a, Q, rep in cases:
        depth[a:a + Q] += 1
        n_events[a:a + Q] += rep
    assert not cols["sum_cost"].any() and cols["depth"].tolist() == depth.tolist() and cols["n_events"].tolist() == n_events.tolist()
    assert not cols["n_samples"].any()
    h_rows = rows.cpu().numpy().view(MAP_ROW).reshape(-1)
    assert total["cost"] == h_rows["cost"].astype(np.int64).sum() == 0 and total["reads_used"] == len(cases) and total["cells"] == n_events.sum()
    # ... and on queries that do not fit: the cost of the table is the sum of the rows' costs (§4.17)
    rng = np.random.default_rng(3)
    qm2 = rng.integers(-100, 101, (40, 90)).astype(np.int16)
    d_q2, d_ql2 = torch.from_numpy(qm2).to("cuda"), torch.full((40,), 90, dtype=torch.int32, device="cuda")
    rows2 = gpu.map.sdtw_dev(d_q2, d_ql2, d_r, want_start=True)
    lo2, hi2, st2 = gpu.align.path_dev(d_q2, d_ql2, d_r, rows2)
    total2, cols2 = pl.to_host(pl.accum_dev(d_q2, d_ql2, d_r, lo2, hi2, st2, pl.new_acc(len(ref))))
    h2 = rows2.cpu().numpy().view(MAP_ROW).reshape(-1)
    assert total2["reads_used"] == 40 and total2["cost"] == h2["cost"].astype(np.int64).sum() > 0
    case = Case(qm2, [90] * 40, ref, lo2.cpu().numpy(), hi2.cpu().numpy(), st2.cpu().numpy())
    assert table_bytes((total2, cols2)) == table_bytes(pileup_ref(case, events=False))


@pytest.mark.gpu
def test_pileup_end_to_end_on_a_synthetic_file(gpu, tmp_path):
    """Pileup.add in two batches, pileup_dev and s5pileup on the six reads of test_align.py, one record corrupt and one read too short: the
    same table, equal to pileup_ref on what align_dev returns"""
    torch, al, pl = gpu.torch, gpu.align, gpu.pileup
    rng = np.random.default_rng(41)
    lengths = [3000, 500, 40, 5000, 1500, 2500]
    recs = [record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
    bad = bytearray(recs[3])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[3] = bytes(bad)
    n, skip, qmax, qmin = len(recs), 2, 100, 20
    ids = [ob.synth_read_id(i) for i in range(n)]
    ids = [i if isinstance(i, bytes) else i.encode() for i in ids]
    levels = rng.normal(500.0, 110.0, 150).astype(np.float32)              # (short: four reads of up to 100 events must share columns)
    ref = quant_ref(levels)
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("# expected levels\n" + "".join("%.9g\n" % v for v in levels))
    kw = dict(skip=skip, qmax=qmax, qmin=qmin)
    # the restatement: on the queries and event rows of the decoded batch and what align_dev returns for it
    dec = gpu.press.decode_to_device(recs)
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:n, 0].contiguous()
    ev_rows, first = gpu.events.events_dev(dec, DNA, "raw")
    q, ql, qst = gpu.map.queries_dev(ev_rows, first, fst, skip, qmax, qmin)
    h_ev, h_first = ev_rows.cpu().numpy().view(EVENT).reshape(-1), first.cpu().numpy()
    qm, qlens = q.cpu().numpy(), ql.cpu().numpy().tolist()
    wev = np.zeros((n, qmax), dtype=EVENT)
    for i in range(n):
        wev[i, :qlens[i]] = h_ev[h_first[i] + skip:h_first[i] + skip + qlens[i]]
    rows, lo, hi, st = al.align_dev(dec, ref, **kw)
    assert st[2] == QUERY_SHORT and st[3] not in (0, QUERY_SHORT, PATH_WIDE, PATH_ROW) and [st[i] for i in (0, 1, 4, 5)] == [0, 0, 0, 0]
    want = pileup_ref(Case(qm, qlens, ref, lo, hi, st, wev))
    total, cols = want
    assert (total["reads_used"], total["reads_skipped"], total["reads_bad"]) == (4, 2, 0) and total["cost"] == rows["cost"][[0, 1, 4, 5]].astype(np.int64).sum()
    assert cols["depth"].max() >= 2 and (cols["n_samples"] >= cols["n_events"]).all()
    # Pileup.add, two batches: the first holds the corrupt record
    with pl.Pileup(ref, **kw) as h:
        with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
            h.add(recs[:4])
        h.abandon()
    h = pl.Pileup(ref, **kw)
    rc, r1, s1 = h.add(recs[:4], raise_on_error=False)
    assert rc == -5 and s1.tolist() == st[:4].tolist() and r1.tolist() == rows[:4].tolist()
    rc, r2, s2 = h.add(recs[4:], raise_on_error=False)                     # the handle stays usable
    assert rc == 0 and s2.tolist() == st[4:].tolist() and r2.tolist() == rows[4:].tolist()
    got = table_bytes(h.close())
    assert got == table_bytes(want), _explain(got, table_bytes(want))
    with pytest.raises(gpu.lib.S5GpuError):
        h.close()
    # pileup_dev on the decoded batch
    acc, dst = pl.pileup_dev(dec, ref, pl.new_acc(len(ref)), **kw)
    got = table_bytes(pl.to_host(acc))
    assert got == table_bytes(want) and dst.cpu().numpy().tolist() == st.tolist(), _explain(got, table_bytes(want))
    # the tool: exit 1, the corrupt read named, the table's lines
    synth_file(tmp_path / "reads.blow5", recs)
    args = ["--skip", str(skip), "--events", str(qmax), "--min-events", str(qmin), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([pl.S5PILEUP, "-K", "4"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[3] in p.stderr and b"short" in p.stderr and b"reads used 4, skipped 2, bad 0" in p.stderr, p.stderr
    assert p.stdout == b"".join(pile_lines(ref, cols)) and len(p.stdout.splitlines()) == int((cols["depth"] >= 1).sum()) > 50
    p = subprocess.run([pl.S5PILEUP, "--min-depth", "2"] + args, capture_output=True, timeout=120)
    deep = pile_lines(ref, cols, 2)
    assert p.returncode == 1 and p.stdout == b"".join(deep) and 0 < len(deep) < int((cols["depth"] >= 1).sum())
    assert subprocess.run([pl.S5PILEUP], capture_output=True).returncode == 2
    assert subprocess.run([pl.S5PILEUP, "--min-depth", "0"] + args, capture_output=True).returncode == 2
    assert subprocess.run([pl.S5PILEUP, "--max-span", "0"] + args, capture_output=True).returncode == 2
    # file_pileup parses the lines back
    t = pl.file_pileup(tmp_path / "reads.blow5", ref_txt, batch=4, raise_on_corrupt=False, **kw)
    at = np.flatnonzero(cols["depth"] >= 1)
    assert t.dtype == pl.PILE_LINE and t["ref_pos"].tolist() == at.tolist() and t["ref_level"].tolist() == ref[at].tolist()
    assert t["depth"].tolist() == cols["depth"][at].tolist() and t["events"].tolist() == cols["n_events"][at].tolist()
    assert t["samples"].tolist() == cols["n_samples"][at].tolist() and t["min"].tolist() == cols["min_q"][at].tolist()
    with pytest.raises(gpu.lib.S5GpuError):
        pl.file_pileup(tmp_path / "reads.blow5", ref_txt, **kw)
