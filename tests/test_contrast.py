"""contrast: per-position level histograms and the two-sample comparison of them (docs/codecs.md §4.23; slow5tools_amd/csrc/contrast_kernels.hip,
behind the plan, the check and the sort of pileup_kernels.hip).

The oracles are hist_ref and contrast_ref in contrast_ref.py: the definitions of §4.23 in int64 numpy and Python integers, tied to
pileup_long_ref of the same case (the bins of a column add up to its n_events, the head to the totals).  Every member is an integer sum, so
the device is held to them byte for byte, whatever the window, the grid, the sort, the segment length, the calls and the streams.  The
headers' plain C++ (pileup_dev.h, and the walk of ragged_dev.h: every segment is resolved by seg_item, as in the kernels) is also compiled for
the CPU, once more under the address and undefined-behaviour sanitizers.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import contrast_ref as cr
from chain_common import DEFAULT_COLS, DEFAULT_HIST_COLS, DEFAULT_HIST_GRID, DEFAULT_SEG, DEFAULT_SORT, PILE_COL, ROOT
from chain_common import host_build, levels_signal, record, synth_file
from chain_common import gpu  # noqa: F401
from contrast_ref import BINS, CONTRAST_ROW, HIST_HEAD, Q0, SHIFT, contrast_lines, contrast_ref, hist_bytes_of, hist_cases, hist_ref, wanted
from dtw_ref import quant_ref
from pileup_ref import LongCase, _first_lo, mixed_case, relay, table_bytes

CALLS = ["s5gpu_pile_hist_bytes", "s5gpu_pile_hist_reset_dev", "s5gpu_pile_hist_accum_long_dev", "s5gpu_pile_contrast_dev", "s5gpu_contrast_open",
         "s5gpu_contrast_add_batch", "s5gpu_contrast_close"]


def _explain(got, want):
    if len(got) != len(want):
        return "%d bytes, %d wanted" % (len(got), len(want))
    g, w = np.frombuffer(got, "<u4"), np.frombuffer(want, "<u4")
    at = np.flatnonzero(g != w)
    return "no difference" if not len(at) else "%d words differ; the first is word %d (column %d, bin %d): %d, %d wanted" % (
        len(at), at[0], (int(at[0]) - 16) // 64, (int(at[0]) - 16) % 64, g[at[0]], w[at[0]])


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_the_contrast_calls_and_the_tool_is_built(tmp_path):
    from slow5tools_amd import _lib, build, contrast

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [1, 5, 13, 7, 8, 10, 4]
    for name in ("HIST_HEAD", "CONTRAST_ROW", "hist_bytes", "new_hist", "hist_accum_long_dev", "hist_accum_dev", "hist_to_host", "contrast_dev", "contrast_whole_dev",
                 "Contrast", "file_contrast"):
        assert hasattr(contrast, name), name
    assert contrast.HIST_HEAD == HIST_HEAD and contrast.CONTRAST_ROW == CONTRAST_ROW
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   'size_t (*a)(uint32_t) = s5gpu_pile_hist_bytes;\n'
                   'int (*b)(void *, uint32_t, int32_t, uint32_t, void *) = s5gpu_pile_hist_reset_dev;\n'
                   'int (*c)(uint32_t, const int16_t *, const uint64_t *, const uint32_t *, uint64_t, uint32_t, const int32_t *, const int32_t *, const int32_t *,'
                   ' void *, size_t, void *, void *) = s5gpu_pile_hist_accum_long_dev;\n'
                   'int (*d)(const void *, const void *, const void *, const void *, uint32_t, s5gpu_pile_contrast_t *, void *) = s5gpu_pile_contrast_dev;\n'
                   'void *(*e)(const s5gpu_event_params_t *, const s5gpu_map_params_t *, const s5gpu_band_params_t *, size_t, const int16_t *, uint32_t, int32_t,'
                   ' uint32_t) = s5gpu_contrast_open;\n'
                   'int (*f)(void *, int, uint32_t, const void *const *, const size_t *, int, int, s5gpu_map_row_t *, s5gpu_ext_row_t *, int32_t *)'
                   ' = s5gpu_contrast_add_batch;\n'
                   'int (*g)(void *, void *, void *, s5gpu_pile_contrast_t *) = s5gpu_contrast_close;\n'
                   'printf("%d %zu %zu\\n", a && b && c && d && e && f && g, sizeof(s5gpu_pile_hist_head_t), sizeof(s5gpu_pile_contrast_t));return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == ["1", "64", "40"]
    # the tool: without arguments its usage (exit 2); with files that do not exist it gets as far as opening the reference
    p = subprocess.run([contrast.S5CONTRAST], capture_output=True)
    assert p.returncode == 2 and b"usage: s5contrast" in p.stderr and b"--shift" in p.stderr and p.stdout == b""
    none = [str(tmp_path / "none.txt"), str(tmp_path / "a.blow5"), str(tmp_path / "b.blow5")]
    p = subprocess.run([contrast.S5CONTRAST, "--q0", "-200", "--shift", "3", "--tile", "64", "--band", "128", "--min-depth", "2"] + none, capture_output=True)
    assert p.returncode == 2 and b"usage" not in p.stderr and b"cannot open" in p.stderr, p.stderr
    for args in (["--shift", "11"], ["--q0", "32768"], ["--q0", "-32769"], ["--tile", "100"], ["--band", "100"], ["--min-depth", "0"], ["--bogus"]):
        p = subprocess.run([contrast.S5CONTRAST] + args + none, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr, (args, p.stderr)
    p = subprocess.run([contrast.S5CONTRAST] + none[:2], capture_output=True)                     # two files only
    assert p.returncode == 2 and b"usage" in p.stderr


def test_hist_bytes():
    from slow5tools_amd import _lib, contrast

    f = _lib.lib().s5gpu_pile_hist_bytes
    assert [f(0), f(1), f(1 << 22), f((1 << 22) + 1)] == [0, 64 + 256, 64 + 256 * (1 << 22), 0]
    assert contrast.hist_bytes(65) == 64 + 256 * 65 and contrast.hist_bytes(0) == 0


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3): the pointers are never dereferenced on the host, so made-up aligned addresses serve"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    P = 1 << 20
    need = L.s5gpu_pileup_long_work_bytes(4, 1000)

    def accum(n=4, q=P, first=P, ql=P, total=1000, R=100, lo=P, hi=P, st=P, work=P, wb=need, hist=P):
        return L.s5gpu_pile_hist_accum_long_dev(n, q, first, ql, total, R, lo, hi, st, work, wb, hist, None)
    assert accum(R=0) == -1 and accum(R=(1 << 22) + 1) == -1 and accum(total=(1 << 40) + 1) == -1
    for name in ("q", "first", "ql", "lo", "hi", "st", "work", "hist"):
        assert accum(**{name: None}) == -1, name
    assert accum(q=P + 1) == -1 and accum(first=P + 4) == -1 and accum(ql=P + 2) == -1 and accum(lo=P + 2) == -1 and accum(hi=P + 1) == -1
    assert accum(st=P + 2) == -1 and accum(work=P + 8) == -1 and accum(hist=P + 8) == -1
    assert accum(wb=need - 1) == -3 and accum(wb=0) == -3
    assert accum(n=0) == 0 and accum(n=0, q=None, first=None, lo=None, work=None, wb=0) == 0      # nothing to do: nothing is launched
    assert accum(n=0, hist=None) == -1 and accum(n=0, R=0) == -1

    def reset(hist=P, R=100, q0=-128, shift=2):
        return L.s5gpu_pile_hist_reset_dev(hist, R, q0, shift, None)
    for kw in (dict(hist=None), dict(hist=P + 8), dict(R=0), dict(R=(1 << 22) + 1), dict(q0=-32769), dict(q0=32768), dict(shift=11)):
        assert reset(**kw) == -1, kw

    def contrast(a=P, b=P, ta=None, tb=None, R=100, out=P):
        return L.s5gpu_pile_contrast_dev(a, b, ta, tb, R, out, None)
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(a=P + 8), dict(b=P + 4), dict(out=P + 4), dict(ta=P), dict(tb=P), dict(ta=P + 8, tb=P), dict(R=0),
               dict(R=(1 << 22) + 1)):
        assert contrast(**kw) == -1, kw
    vp = C.c_void_p
    h_ref = np.zeros(100, dtype=np.int16)

    def opened(mp=(0, 64, 10, 32.0, 127, 1), bp=(0, 10, 1 << 20, 256, 512, 127, 32.0), ev=(3, 6, 1.4, 9.0, 0.2), R=100, ref=True, bp_null=False, q0=-128, shift=2):
        e, m, b = _lib.EventParams(*ev), _lib.MapParams(*mp), _lib.BandParams(*bp)
        ref_p = (np.zeros(R, dtype=np.int16) if R > 100 else h_ref).ctypes.data_as(vp) if ref else None
        h = L.s5gpu_contrast_open(C.byref(e), C.byref(m), None if bp_null else C.byref(b), 0, ref_p, R, q0, shift)
        return h, L.s5gpu_last_error()
    for kw in (dict(bp_null=True), dict(bp=(0, 10, 1 << 20, 100, 512, 127, 32.0)), dict(bp=(1, 10, 1 << 20, 256, 512, 127, 32.0)), dict(mp=(0, 0, 1, 32.0, 127, 1)),
               dict(R=0), dict(R=(1 << 22) + 1), dict(ref=False), dict(q0=32768), dict(q0=-32769), dict(shift=11)):
        h, why = opened(**kw)
        assert h is None and why.startswith(b"s5gpu_contrast_open:") and b"device" not in why, (kw, why)
    assert L.s5gpu_contrast_add_batch(None, 0, 0, None, None, 1, 1, None, None, None) == -1
    assert L.s5gpu_contrast_close(None, None, None, None) == 0


def test_the_options_refuse_bad_values():
    from slow5tools_amd import _lib

    L = _lib.lib()
    for key, bad, good in ((b"pile_hist_cols", (-1, 1, 8, 15, 17, 48, 96, 512, 1024), (0, 16, 32, 64, 128, 256, DEFAULT_HIST_COLS)),
                           (b"pile_hist_grid", (0, -1, 1025), (1, 7, 1024, DEFAULT_HIST_GRID))):
        for v in bad:
            assert L.s5gpu_set_option(key, v) == -1, (key, v)
        for v in good:                                                     # (the defaults last)
            assert L.s5gpu_set_option(key, v) == 0, (key, v)
    for key, v in ((b"pileup_long_seg", DEFAULT_SEG), (b"pileup_long_cols", DEFAULT_COLS), (b"pileup_lds_cols", DEFAULT_COLS)):   # the old keys keep their meaning
        assert L.s5gpu_set_option(key, v) == 0
    assert L.s5gpu_set_option(b"pile_hist_rows", 1) == -1


def test_the_restatements():
    # hand-made: two reads on 4 columns, default bins (bin = (q + 128) >> 2)
    q = np.array([-128, -125, 0, 127, 200], dtype=np.int16)
    lo, hi = np.array([0, 1, 2, 1, 1], dtype=np.int32), np.array([1, 1, 3, 1, 2], dtype=np.int32)
    head, counts = hist_ref(LongCase(q, [0, 3, 5], [3, 2], [0, 0, 0, 0], lo, hi))
    want = np.zeros((4, 64), np.int64)
    for j, b in ((0, 0), (1, 0), (1, 0), (2, 32), (3, 32), (1, 63), (1, 63), (2, 63)):
        want[j, b] += 1
    assert counts.tolist() == want.tolist() and tuple(head)[:8] == (8, 2, 0, 0, 4, -128, 2, 64)
    assert cr.bin_of([-32768, -129, -128, -125, -124, 123, 124, 127, 128, 32767], -128, 2).tolist() == [0, 0, 0, 0, 1, 62, 63, 63, 63, 63]
    assert cr.bin_of([32766, 32767], 32767, 0).tolist() == [0, 0] and cr.bin_of([-32768, 32767], -32768, 10).tolist() == [0, 63]
    # every case: the invariants against pileup_long_ref are asserted inside hist_ref
    for name in hist_cases():
        assert len(wanted(name)) == 64 + 256 * hist_cases()[name][0].R
    # the comparison: identical, disjoint, empty; the tie goes to the smallest bin; the sign both ways
    rng = np.random.default_rng(5)
    A = rng.integers(0, 50, (6, 64))
    A[5] = 0
    B = A.copy()
    B[1] = 0
    B[1, 40:] = rng.integers(1, 9, 24)
    A[1, 40:] = 0                                                           # column 1: A below bin 40, B from it on
    A[1, 39] = 5
    A[2], B[2] = 0, 0
    A[2, [3, 9]], B[2, [5, 9]] = [1, 1], [1, 1]                              # cA - cB = 1/2 at bins 3 and 4: the tie
    A[3], B[3] = B[2], A[2]
    B[4] = 0
    rows = contrast_ref(A, B)
    nn = rows["n_a"].astype(object) * rows["n_b"].astype(object)
    assert rows["ks_num"][0] == 0 and rows["ov_num"][0] == nn[0] and rows["flags"][0] == 0 and rows["ks_bin"][0] == 0
    assert rows["ks_num"][1] == nn[1] and rows["ov_num"][1] == 0 and rows["ks_bin"][1] == 39 and rows["flags"][1] == 4
    assert (rows["ks_bin"][2], rows["flags"][2], rows["ks_num"][2], rows["ov_num"][2]) == (3, 4, 2, 2) and (rows["ks_bin"][3], rows["flags"][3]) == (3, 0)
    assert (rows["flags"][4], rows["n_b"][4], rows["ks_num"][4], rows["med_b"][4]) == (2, 0, 0, 0) and rows["flags"][5] == 3
    big = np.zeros((2, 64), np.int64)
    big[0, 7], big[1, 7] = 2 ** 31 - 1, 2 ** 31
    other = np.zeros((2, 64), np.int64)
    other[:, 9] = [2 ** 31 - 1, 5]
    rows = contrast_ref(big, other)
    assert rows["ks_num"][0] == (2 ** 31 - 1) ** 2 and rows["ov_num"][0] == 0 and rows["flags"][0] == 4 and (rows["med_a"][0], rows["med_b"][0]) == (7, 9)
    assert (rows["flags"][1], rows["ks_num"][1], rows["ov_num"][1], rows["n_a"][1], rows["med_a"][1]) == (8, 0, 0, 2 ** 31, 7)
    assert (contrast_ref(big, other, heads_agree=False)["flags"] == 128).all()


HIST_HOST = r'''
// The histogram code of pileup_dev.h on the CPU, with plain adds in place of the atomics: what k_pileup_long_plan, _check, the sort and
// k_pile_hist_accum do with it, every table allocated at exactly its size, the segments visited in a shuffled order (or in the sort's),
// each resolved by seg_item of ragged_dev.h.
// in.bin: n, R, S, cols, wlo, sort, seed, q0, shift, pad (uint32), total_rows (uint64), then first, qlen, status, queries, lo, hi;
// out.bin: the histogram's bytes.
#define S5_PILEUP_HOST
#include "pileup_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace pilek;
struct HostOps {
    static void add32(uint32_t *p, uint32_t v) { *p += v; }
    static void add32_win(uint32_t *p, uint32_t v) { *p += v; }
};
template <class T>
static T *get(FILE *f, size_t k) {                                          // exactly k elements
    T *p = (T *)malloc(k ? k * sizeof(T) : 1);
    if (!p || (k && fread(p, sizeof(T), k, f) != k)) abort();
    return p;
}
static uint64_t g_rand;
static uint64_t rnd() { g_rand = g_rand * 6364136223846793005ull + 1442695040888963407ull; return g_rand >> 33; }
static void shuffle(uint64_t *v, uint64_t k) { for (uint64_t i = k; i > 1; i--) { const uint64_t j = rnd() % i, t = v[i - 1]; v[i - 1] = v[j]; v[j] = t; } }

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t h[10];
    uint64_t total_rows;
    if (!f || !o || fread(h, 4, 10, f) != 10 || fread(&total_rows, 8, 1, f) != 1) return 1;
    const uint32_t n = h[0], R = h[1], S = h[2], cols = h[3], sort = h[5], shift = h[8];
    const int32_t q0 = (int32_t)h[7];
    g_rand = h[6];
    uint64_t *first = get<uint64_t>(f, (size_t)n + 1);
    uint32_t *qlen = get<uint32_t>(f, n);
    int32_t *status = get<int32_t>(f, n);
    int16_t *q = get<int16_t>(f, total_rows);
    int32_t *lo = get<int32_t>(f, total_rows), *hi = get<int32_t>(f, total_rows);
    const PileLongArgs A = {n, q, first, qlen, total_rows, nullptr, R, lo, hi, status, nullptr, 0u, nullptr, nullptr};
    const uint64_t cap = long_order_cap(n, total_rows);
    uint32_t hist[LONG_KEYS], cursor[LONG_KEYS], *verdict = (uint32_t *)malloc(n ? 4ull * n : 1);
    uint64_t *P = (uint64_t *)malloc(8ull * (n + 1ull)), *order = (uint64_t *)malloc(cap ? 8 * cap : 1);   // the work area's parts, each at exactly its size
    const LongPtrs L = {verdict, P, hist, cursor, order, cap};
    memset(hist, 0, sizeof hist);
    P[0] = 0;
    for (uint32_t k = 0; k < n; k++) {
        verdict[k] = long_verdict(first[k], first[k + 1], qlen[k], status[k], total_rows, 0u);
        P[k + 1] = P[k] + (verdict[k] == V_USED ? segs_of(qlen[k], S) : 0u);
    }
    const uint64_t total = P[n];
    uint64_t *list = (uint64_t *)malloc(total ? 8 * total : 1);
    for (uint64_t g = 0; g < total; g++) list[g] = g;
    shuffle(list, total);
    const bool sorted = sort && total <= cap;
    for (uint64_t x = 0; x < total; x++) {                                  // every segment through seg_item, the kernels' resolver
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, false, list[x], &g)) return 4;
        if (!seg_rows_ok(g.r0, g.r1, 0, 1, lo + first[g.k], hi + first[g.k], R)) verdict[g.k] |= V_BAD;
        if (sorted) hist[seg_key(lo[first[g.k] + g.r0], R)]++;
    }
    if (sorted) {
        uint32_t at = 0;
        for (uint32_t b = 0; b < LONG_KEYS; b++) { cursor[b] = at; at += hist[b]; }
        for (uint64_t x = 0; x < total; x++) {
            Seg g = seg_none(n);
            if (!seg_item(A, S, L, false, list[x], &g)) return 4;
            const uint64_t pos = cursor[seg_key(lo[first[g.k] + g.r0], R)]++;
            if (pos >= cap) return 5;
            order[pos] = (uint64_t)g.k << 32 | g.s;
        }
    } else {
        shuffle(list, total);
    }
    // the cells: a table of exactly R columns and a window of exactly cols; the items of the ordered list, or of P's order shuffled
    uint32_t *table = (uint32_t *)calloc(R ? (size_t)R * HIST_BINS : 1, 4), *win = (uint32_t *)calloc(cols ? (size_t)cols * HIST_BINS : 1, 4);
    Window W;
    W.lo = h[4]; W.cols = cols;
    s5gpu_pile_hist_head_t T;
    memset(&T, 0, sizeof T);
    T.R = R; T.q0 = q0; T.shift = shift; T.bins = HIST_BINS;
    for (uint64_t x = 0; x < total; x++) {
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, sorted, sorted ? x : list[x], &g)) return 4;
        if (verdict[g.k] != V_USED) continue;
        hist_seg_cells<HostOps>(g.r0, g.r1, 0, 1, lo + first[g.k], hi + first[g.k], q + first[g.k], q0, shift, R, W, win, table, &T.cells);
    }
    for (uint32_t t = 0; t < cols * HIST_BINS; t++) {
        hist_flush_word<HostOps>(t, W, win, table, R);
        if (win[t]) return 2;                                              // a cell went to a slot that stands for no column
    }
    for (int32_t v = -32768; v <= 32767; v++) if (hist_bin(v, q0, shift) >= HIST_BINS || hist_bin(v, q0, 31u) >= HIST_BINS) return 3;
    for (uint32_t k = 0; k < n; k++) {
        if (verdict[k] & V_SKIPPED) T.reads_skipped++;
        else if (verdict[k] & V_BAD) T.reads_bad++;
        else T.reads_used++;
    }
    fwrite(&T, sizeof T, 1, o);
    fwrite(table, 4, (size_t)R * HIST_BINS, o);
    free(table); free(win); free(order); free(list); free(P); free(verdict); free(first); free(qlen); free(status); free(q); free(lo); free(hi);
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _run_host(exe, tmp_path, case, q0, shift, S=64, cols=0, wlo=0, sort=0, seed=1):
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<7Ii2IQ", case.n, case.R, S, cols, wlo, sort, seed, q0, shift, 0, case.total))
        for a in (case.first, case.qlen, case.status, case.q, case.lo, case.hi):
            fh.write(a.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return (tmp_path / "out.bin").read_bytes()


def run_hist_header_on_the_cpu(tmp_path, extra=()):
    exe = host_build(tmp_path, "hist_host", HIST_HOST, ["-O1", "-g", "-std=c++17", "-Wall"], extra)
    for name, (case, q0, shift) in hist_cases().items():
        if extra and case.total > 100000:
            continue
        want = wanted(name)
        # without a window; a window of 16 columns at the kernel's anchor, at column 0 and hanging over the table's end; shuffled and sorted
        for cols, wlo, sort, S, seed in ((0, 0, 0, 64, 1), (16, _first_lo(case), 1, 64, 2), (16, 0, 0, 256, 3), (16, max(case.R - 10, 0), 1, 1024, 4),
                                         (256, max(case.R - 10, 0), 0, 64, 5)):
            got = _run_host(exe, tmp_path, case, q0, shift, S, cols, wlo, sort, seed)
            assert got == want, (name, cols, wlo, sort, S, _explain(got, want))


def test_the_header_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """hist_bin, hist_col_add, hist_row_cells, hist_seg_cells, the window's slot and hist_flush_word of pileup_dev.h as g++ compiles them"""
    run_hist_header_on_the_cpu(tmp_path)


def test_the_header_code_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: every table is allocated at exactly its size"""
    run_hist_header_on_the_cpu(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _planted_condition(rows):
    top, d = cr.largest_d(rows, 5, 8)
    assert len(top) == 5 and all(cr.PLANTED_COLS[0] <= j <= cr.PLANTED_COLS[1] for j in top), (top, [float(d[j]) for j in top])
    return top, d


def test_the_planted_case_at_the_query_level():
    """among the columns with at least 8 cells a side, the five of largest D all lie in the ten columns whose levels were shifted"""
    ref, sides = cr.planted()
    paths = cr.planted_paths()
    A, B = (hist_ref(cr.planted_case(ref, sides[s], paths[s])) for s in (0, 1))
    rows = contrast_ref(A[1], B[1])
    top, d = _planted_condition(rows)
    rest = sorted(float(v) for j, v in d.items() if not cr.PLANTED_COLS[0] <= j <= cr.PLANTED_COLS[1])
    print("planted: top", top, [float(d[j]) for j in top], "median D elsewhere %.3f" % rest[len(rest) // 2])


# ---------------------------------------------------------------------------------------------------------------- gpu

def _options(env, cols=DEFAULT_HIST_COLS, grid=DEFAULT_HIST_GRID, sort=DEFAULT_SORT, seg=64):
    for key, v in ((b"pile_hist_cols", cols), (b"pile_hist_grid", grid), (b"pileup_long_sort", sort), (b"pileup_long_seg", seg)):
        env.lib.check(env.L.s5gpu_set_option(key, v), key.decode())


class Hist:
    """a histogram of R columns on the device between two guards of 64 bytes of 0x5A, reset"""

    def __init__(self, env, R, q0=Q0, shift=SHIFT):
        self.env, self.R, self.nb = env, R, 64 + 256 * R
        self.t = env.torch.full((self.nb + 128,), 0x5A, dtype=env.torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + 64
        assert self.ptr % 16 == 0 and env.L.s5gpu_pile_hist_bytes(R) == self.nb
        env.lib.check(env.L.s5gpu_pile_hist_reset_dev(self.ptr, R, q0, shift, None), "s5gpu_pile_hist_reset_dev")

    def bytes(self):
        self.env.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:64] == 0x5A).all() and (h[-64:] == 0x5A).all(), "a guard of the histogram was written"
        return h[64:-64].tobytes()


def _accum(env, hist, case, stream=None, sync=True, short=0, want_rc=0):
    """THE way into s5gpu_pile_hist_accum_long_dev here: the inputs uploaded, a work area of exactly the size asked for between guards, the call
    made on `stream`, and afterwards the guards and every input checked.  short: the bytes the call is told are missing."""
    torch = env.torch
    host = [case.q, case.first.view(np.int64), case.qlen.view(np.int32), case.lo, case.hi, case.status]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in host]
    need = env.L.s5gpu_pileup_long_work_bytes(case.n, case.total)
    work = torch.full((need + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if t.numel() else None for t in dev]
    rc = env.L.s5gpu_pile_hist_accum_long_dev(case.n, ptr[0], ptr[1], ptr[2], case.total, case.R, ptr[3], ptr[4], ptr[5], work.data_ptr() + 64, need - short, hist.ptr,
                                              C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == want_rc, (rc, env.L.s5gpu_last_error())

    def check():
        for t, a in zip(dev, host):
            assert np.array_equal(t.cpu().numpy(), a), "an input was written"
        w = work.cpu().numpy()
        assert (w[:64] == 0x5A).all() and (w[-64:] == 0x5A).all(), "a guard of the work area was written"
        if want_rc != 0:
            assert (w == 0x5A).all(), "the work area was written by a call that was refused"
        return hist.bytes()
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


def _hist(env, name, **opt):
    case, q0, shift = hist_cases()[name]
    _options(env, **opt)
    try:
        return _accum(env, Hist(env, case.R, q0, shift), case)
    finally:
        _options(env, seg=DEFAULT_SEG)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hist_cases()))
def test_the_case_list_is_exact(gpu, name):
    want = wanted(name)
    for opt in (dict(), dict(cols=16, sort=0), dict(seg=DEFAULT_SEG)):
        got = _hist(gpu, name, **opt)
        assert got == want, (opt, _explain(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges R=300 q0=-128 shift=2", "edges R=65 q0=0 shift=0", "seams", "piling"])
def test_the_options_do_not_change_a_byte(gpu, name):
    want = wanted(name)
    for cols in (0, 16, 256):
        for grid in (1, DEFAULT_HIST_GRID):
            for sort in (0, 1):
                for seg in (64, 1024):
                    got = _hist(gpu, name, cols=cols, grid=grid, sort=sort, seg=seg)
                    assert got == want, (cols, grid, sort, seg, _explain(got, want))


@pytest.mark.gpu
def test_two_calls_on_two_streams_and_a_short_work_area(gpu):
    torch = gpu.torch
    case = mixed_case(129, 200)
    whole = relay(case)
    want = hist_bytes_of(hist_ref(whole))
    a, b = relay(case.part(0, 90)), relay(case.part(90, 200))
    hist = Hist(gpu, case.R)
    _options(gpu)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        checks = [_accum(gpu, hist, a, stream=s1, sync=False), _accum(gpu, hist, b, stream=s2, sync=False)]
        torch.cuda.synchronize()
        got = [f() for f in checks][-1]
        assert got == want, _explain(got, want)
        # a work area one byte short: S5GPU_ERR_NOMEM, and neither the histogram nor the work area is touched
        assert _accum(gpu, hist, a, short=1, want_rc=-3) == want
    finally:
        _options(gpu, seg=DEFAULT_SEG)


@pytest.mark.gpu
def test_a_fixed_pitch_batch_equals_the_ragged_call(gpu):
    torch, ct = gpu.torch, gpu.contrast
    case = mixed_case(129, 200)
    want = hist_bytes_of(hist_ref(relay(case, seed=3)))

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    hist = ct.hist_accum_dev(dev(case.qm), dev(case.qlen.view(np.int32)), dev(case.lo), dev(case.hi), dev(case.status), ct.new_hist(case.R))
    head, counts = ct.hist_to_host(hist)
    got = hist_bytes_of((head, counts))
    assert got == want, _explain(got, want)
    assert _accum(gpu, Hist(gpu, case.R), relay(case)) == want


def _upload_hist(env, counts, q0=Q0, shift=SHIFT, R=None):
    head = np.zeros(1, dtype=HIST_HEAD)
    head[0] = (int(np.asarray(counts, dtype=object).sum()) % 2 ** 64, 0, 0, 0, len(counts) if R is None else R, q0, shift, BINS, (0, 0))
    return env.torch.from_numpy(np.frombuffer(hist_bytes_of((head[0], counts)), dtype=np.uint8).copy()).to("cuda")


def _upload_acc(env, depth, n_events):
    cols = np.zeros(len(depth), dtype=PILE_COL)
    cols["depth"], cols["n_events"], cols["min_q"], cols["max_q"] = depth, n_events, 32767, -32768
    return env.torch.from_numpy(np.frombuffer(bytes(64) + cols.tobytes(), dtype=np.uint8).copy()).to("cuda"), cols


def _rows(env, *a):
    out = env.contrast.rows_to_host(env.contrast.contrast_dev(*a))
    env.torch.cuda.synchronize()
    return out


def _same_rows(got, want):
    bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
    assert not bad, (bad[:5], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
def test_the_comparison_on_hand_made_histograms(gpu):
    rng = np.random.default_rng(23)
    # R = 1; identical, disjoint and one-sided empty columns; the tie; the sign both ways; the top of the range and one above it
    one = rng.integers(0, 9, (1, 64))
    _same_rows(_rows(gpu, _upload_hist(gpu, one), _upload_hist(gpu, one[:, ::-1].copy())), contrast_ref(one, one[:, ::-1]))
    A = rng.integers(0, 50, (10, 64)).astype(np.int64)
    B = A.copy()
    A[1, 40:], B[1, :40] = 0, 0
    A[2], B[2] = 0, 0
    A[2, [3, 9]], B[2, [5, 9]] = [1, 1], [1, 1]
    A[3], B[3] = B[2].copy(), A[2].copy()
    B[4] = 0
    A[5] = 0
    A[6], B[6] = 0, 0
    A[7], B[7] = 0, 0
    A[7, 7], B[7, 7] = 2 ** 31 - 1, 2 ** 31 - 1
    A[8], B[8] = 0, 0
    A[8, 7], B[8, 9] = 2 ** 31 - 1, 2 ** 31 - 1
    A[9], B[9] = 0, 0
    A[9, 7], B[9, 7] = 2 ** 31, 2 ** 31
    want = contrast_ref(A, B)
    assert want["flags"].tolist() == [0, 4, 4, 0, 2, 1, 3, 0, 4, 8] and want["ks_bin"][2] == want["ks_bin"][3] == 3 and want["ks_num"][8] == (2 ** 31 - 1) ** 2
    assert want["ov_num"][7] == (2 ** 31 - 1) ** 2 and (want["ks_num"][9], want["ov_num"][9], want["n_a"][9]) == (0, 0, 2 ** 31)
    ha, hb = _upload_hist(gpu, A), _upload_hist(gpu, B)
    _same_rows(_rows(gpu, ha, hb), want)
    _same_rows(_rows(gpu, ha, ha), contrast_ref(A, A))                     # (the same histogram on both sides)
    # tables that agree, and that do not
    na, nb = A.sum(axis=1), B.sum(axis=1)
    ea, eb = np.minimum(na, 2 ** 32 - 1), np.minimum(nb, 2 ** 32 - 1)
    ta, ca = _upload_acc(gpu, np.minimum(ea, 7), ea)
    tb, cb = _upload_acc(gpu, np.minimum(eb, 5), eb)
    want = contrast_ref(A, B, ca, cb)
    assert not (want["flags"] & 48).any() and want["depth_a"].max() == 7
    _same_rows(_rows(gpu, ha, hb, ta, tb), want)
    ea[0] += 1
    eb[3] -= 1
    ta, ca = _upload_acc(gpu, np.minimum(ea, 7), ea)
    tb, cb = _upload_acc(gpu, np.minimum(eb, 5), eb)
    want = contrast_ref(A, B, ca, cb)
    assert (want["flags"] & 48).tolist() == [16, 0, 0, 32, 0, 0, 0, 0, 0, 0]
    _same_rows(_rows(gpu, ha, hb, ta, tb), want)
    # heads that disagree: q0, shift, R
    for kw in (dict(q0=-127), dict(shift=3), dict(R=11)):
        got = _rows(gpu, ha, _upload_hist(gpu, B, **kw))
        _same_rows(got, contrast_ref(A, B, heads_agree=False))
    # 1000 random columns: sparse and dense, small and large counts
    A = rng.integers(0, 2 ** rng.integers(1, 26, (1000, 1)), (1000, 64)) * (rng.random((1000, 64)) < rng.random((1000, 1)))
    B = rng.integers(0, 2 ** rng.integers(1, 26, (1000, 1)), (1000, 64)) * (rng.random((1000, 64)) < rng.random((1000, 1)))
    B[::7] = np.roll(A[::7], 1, axis=1)
    _same_rows(_rows(gpu, _upload_hist(gpu, A), _upload_hist(gpu, B)), contrast_ref(A, B))


@pytest.mark.gpu
def test_the_planted_case_through_the_device(gpu):
    """extend.band_dev -> hist_accum_long_dev -> contrast_dev on the planted case: the restatement fed with the device's lo / hi, byte for byte,
    and the five-largest condition on the device's rows"""
    torch, ex, ct = gpu.torch, gpu.extend, gpu.contrast
    ref, sides = cr.planted()
    p = ex.BandParams(0, 1, 1 << 20, 64, 128)

    def dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")
    hists, wants = [], []
    for reads in sides:
        Q = [len(q) for q, _ in reads]
        first = np.concatenate(([0], np.cumsum(Q))).astype(np.int64)
        q, ql, st = dev(np.concatenate([q for q, _ in reads])), dev(Q, np.int32), dev(np.zeros(len(Q)), np.int32)
        rows, lo, hi = ex.band_dev(q, dev(first), ql, dev(ref), dev([a for _, a in reads], np.int32), st, p, None)
        status = (rows[:, 3] >> 32).to(torch.int32)
        hists.append(ct.hist_accum_long_dev(q, dev(first), ql, lo, hi, status, ct.new_hist(len(ref))))
        h_lo, h_hi = lo.cpu().numpy(), hi.cpu().numpy()
        assert status.cpu().numpy().tolist() == [0] * len(Q)
        wants.append(hist_ref(cr.planted_case(ref, reads, [(h_lo[first[k]:first[k + 1]], h_hi[first[k]:first[k + 1]]) for k in range(len(Q))])))
    for h, w in zip(hists, wants):
        got = hist_bytes_of(ct.hist_to_host(h))
        assert got == hist_bytes_of(w), _explain(got, hist_bytes_of(w))
    rows = ct.rows_to_host(ct.contrast_dev(hists[0], hists[1]))
    _same_rows(rows, contrast_ref(wants[0][1], wants[1][1]))
    _planted_condition(rows)


@pytest.fixture(scope="module")
def files(gpu):
    """two small synthetic files, made as test_pileup_long's chain fixture makes its records (one read a side too short for a query), and what
    contrast_whole_dev makes of them"""
    rng = np.random.default_rng(4023)
    levels = rng.normal(500.0, 110.0, 3500).astype(np.float32)
    ref = quant_ref(levels)
    recs = [[record(10 * s + i, levels_signal(n, rng)) for i, n in enumerate(lengths)] for s, lengths in enumerate(([30000, 100, 26000, 28000], [27000, 31000, 100]))]
    kw = dict(skip=2, qmax=100, qmin=20, tile_rows=64, band=128)
    env = type("Files", (), {})()
    env.recs, env.levels, env.ref, env.kw = recs, levels, ref, kw
    rows, accs, hists = gpu.contrast.contrast_whole_dev(gpu.press.decode_to_device(recs[0]), gpu.press.decode_to_device(recs[1]), ref, **kw)
    env.rows = gpu.contrast.rows_to_host(rows)
    env.accs = [gpu.pileup.to_host(a) for a in accs]
    env.hists = [gpu.contrast.hist_to_host(h) for h in hists]
    return env


@pytest.mark.gpu
def test_the_chain_and_the_handle(gpu, files):
    ct, pl = gpu.contrast, gpu.pileup
    # the device chain against the restatement: the rows of the histograms and the tables it left, and the invariants of the two
    want = contrast_ref(files.hists[0][1], files.hists[1][1], files.accs[0][1], files.accs[1][1])
    _same_rows(files.rows, want)
    assert not (files.rows["flags"] & ~np.uint16(7)).any() and ((files.rows["depth_a"] >= 1) & (files.rows["depth_b"] >= 1)).sum() > 100
    for s in (0, 1):
        head, counts = files.hists[s]
        total, cols = files.accs[s]
        assert counts.sum(axis=1).tolist() == cols["n_events"].tolist() and head["cells"] == total["cells"]
        assert (head["reads_used"], head["reads_skipped"], head["reads_bad"]) == (total["reads_used"], total["reads_skipped"], total["reads_bad"]) == ((3, 1, 0), (2, 1, 0))[s]
    tables = [table_bytes(a) for a in files.accs]
    # the handle: a batch a side, and two
    for split in (None, 2):
        with ct.Contrast(files.ref, **files.kw) as h:
            for s in (1, 0):
                parts = [files.recs[s]] if split is None else [files.recs[s][:split], files.recs[s][split:]]
                for part in parts:
                    rc, map_rows, ext_rows, status = h.add(s, part)
                    assert rc == 0 and len(ext_rows) == len(part)
            rows, a, b = h.close()
        _same_rows(rows, files.rows)
        assert [table_bytes(a), table_bytes(b)] == tables
    # ... whose tables are PileupWhole's of the same files
    for s in (0, 1):
        with pl.PileupWhole(files.ref, **files.kw) as h:
            h.add(files.recs[s])
            assert table_bytes(h.close()) == tables[s]
    # a corrupt record: -5, the rest accumulated, the handle usable
    recs = list(files.recs[0])
    bad = bytearray(recs[2])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[2] = bytes(bad)
    h = ct.Contrast(files.ref, **files.kw)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        h.add(0, recs)
    h.abandon()
    h = ct.Contrast(files.ref, **files.kw)
    rc, _, ext_rows, status = h.add(0, recs, raise_on_error=False)
    assert rc == -5 and status[2] != 0 and ext_rows["qlen"][2] == 0
    assert gpu.L.s5gpu_contrast_add_batch(h._h, 2, 0, None, None, 1, 1, None, None, None) == -1
    rc, _, _, _ = h.add(1, files.recs[1])
    assert rc == 0
    rows, (ta, ca), (tb, cb) = h.close()
    assert (ta["reads_used"], ta["reads_skipped"]) == (2, 2) and table_bytes((tb, cb)) == tables[1]
    with pl.PileupWhole(files.ref, **files.kw) as p:
        p.add(recs, raise_on_error=False)
        assert table_bytes(p.close()) == table_bytes((ta, ca))
    assert rows["n_a"].tolist() == ca["n_events"].tolist() and rows["n_b"].tolist() == files.rows["n_b"].tolist() and not (rows["flags"] & 48).any()


@pytest.mark.gpu
def test_the_tool_and_file_contrast(gpu, files, tmp_path):
    ct = gpu.contrast
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("".join("%.9g\n" % v for v in files.levels))
    for s, name in enumerate(("a.blow5", "b.blow5")):
        synth_file(tmp_path / name, files.recs[s])
    kw = files.kw
    paths = [str(ref_txt), str(tmp_path / "a.blow5"), str(tmp_path / "b.blow5")]
    args = ["--skip", str(kw["skip"]), "--events", str(kw["qmax"]), "--min-events", str(kw["qmin"]), "--tile", str(kw["tile_rows"]), "--band", str(kw["band"])]
    p = subprocess.run([ct.S5CONTRAST, "-K", "3"] + args + paths, capture_output=True, timeout=120)
    assert p.returncode == 0 and b"a.blow5: reads used 3, skipped 1, bad 0" in p.stderr and b"b.blow5: reads used 2, skipped 1, bad 0" in p.stderr, p.stderr
    want = contrast_lines(files.ref, files.rows, files.accs[0][1], files.accs[1][1])
    assert p.stdout == b"".join(want) and len(want) > 100
    p = subprocess.run([ct.S5CONTRAST, "-K", "3", "--min-depth", "2"] + args + paths, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(contrast_lines(files.ref, files.rows, files.accs[0][1], files.accs[1][1], 2)) and len(p.stdout) < len(b"".join(want))
    t = ct.file_contrast(paths[1], paths[2], paths[0], batch=3, tile_rows=kw["tile_rows"], band=kw["band"], skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"])
    at = np.flatnonzero((files.rows["depth_a"] >= 1) & (files.rows["depth_b"] >= 1))
    assert t["ref_pos"].tolist() == at.tolist() and t["events_a"].tolist() == files.rows["n_a"][at].tolist() and t["depth_b"].tolist() == files.rows["depth_b"][at].tolist()
    assert t["med_a"].tolist() == (Q0 + (files.rows["med_a"][at].astype(np.int64) << SHIFT)).tolist() and (t["ks_d"] <= 1.0).all() and (t["tv"] >= 0.0).all()
