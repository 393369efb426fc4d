"""sites: per-read levels at chosen reference columns, each held against a control histogram (docs/codecs.md §4.25;
slow5tools_amd/csrc/sites_kernels.hip, behind the plan and the check of pileup_kernels.hip).

The oracles are cells_ref and score_ref in sites_ref.py: the definitions of §4.25 in int64 numpy and Python integers, tied to hist_ref and
pileup_long_ref of the same case (the cells of a site add up to its column of the histogram, the sums to the table's sum_q).  Every member is
an integer sum or a minimum, so the device is held to them byte for byte, whatever the segment length, the grid, the calls and the streams.
The header's plain C++ (sites_dev.h, and the walk of ragged_dev.h: every segment is resolved by seg_item, as in the kernels) is also compiled
for the CPU, once more under the address and undefined-behaviour sanitizers.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import contrast_ref as cr
import oracle_bind as ob
import sites_ref as sr
from chain_common import DEFAULT_GRID, DEFAULT_SEG, EXT_ROW, ROOT, host_build, levels_signal, record, synth_file
from chain_common import gpu  # noqa: F401
from contrast_ref import BINS, HIST_HEAD, Q0, SHIFT, hist_bytes_of, hist_cases, hist_ref
from dtw_ref import quant_ref
from pileup_ref import LongCase, long_cases, mixed_case, relay
from sites_ref import ROW_NONE, SITE_CELL, SITE_SCORE, cells_ref, score_ref, site_lists, verdicts_ref, wanted

CALLS = ["s5gpu_site_cells_long_dev", "s5gpu_site_score_dev", "s5gpu_sites_open", "s5gpu_sites_set_refine", "s5gpu_sites_add_control", "s5gpu_sites_set_control",
         "s5gpu_sites_add_batch", "s5gpu_sites_close"]
SETTINGS = ((64, 1), (64, DEFAULT_GRID), (256, 7), (1024, DEFAULT_GRID))   # pileup_long_seg, pileup_long_grid


def _explain(got, want):
    g, w = np.asarray(got), np.asarray(want)
    if g.shape != w.shape:
        return "shape %s, %s wanted" % (g.shape, w.shape)
    bad = np.argwhere(g != w)
    return "no difference" if not len(bad) else "%d entries differ; the first is [site %d, read %d]: %s, %s wanted" % (
        len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_the_sites_calls_and_the_tool_is_built(tmp_path):
    from slow5tools_amd import _lib, build, sites

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [16, 8, 10, 2, 7, 2, 10, 2]
    for name in ("SITE_CELL", "SITE_SCORE", "check_sites", "cells_long_dev", "cells_dev", "score_dev", "cells_to_host", "scores_to_host", "tail", "sites_whole_dev",
                 "Sites", "file_sites"):
        assert hasattr(sites, name), name
    assert sites.SITE_CELL == SITE_CELL and sites.SITE_SCORE == SITE_SCORE
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   'int (*a)(uint32_t, const int16_t *, const uint64_t *, const uint32_t *, uint64_t, uint32_t, const int32_t *, const int32_t *, const int32_t *,'
                   ' const uint32_t *, uint32_t, void *, size_t, s5gpu_site_cell_t *, uint32_t *, void *) = s5gpu_site_cells_long_dev;\n'
                   'int (*b)(const s5gpu_site_cell_t *, uint32_t, const uint32_t *, uint32_t, const void *, uint32_t, s5gpu_site_score_t *, void *) = s5gpu_site_score_dev;\n'
                   'void *(*c)(const s5gpu_event_params_t *, const s5gpu_map_params_t *, const s5gpu_band_params_t *, size_t, const int16_t *, uint32_t,'
                   ' const uint32_t *, uint32_t, int32_t, uint32_t) = s5gpu_sites_open;\n'
                   'int (*d)(void *, const s5gpu_refine_params_t *) = s5gpu_sites_set_refine;\n'
                   'int (*e)(void *, uint32_t, const void *const *, const size_t *, int, int, int32_t *) = s5gpu_sites_add_control;\n'
                   'int (*f)(void *, const void *) = s5gpu_sites_set_control;\n'
                   'int (*g)(void *, uint32_t, const void *const *, const size_t *, int, int, s5gpu_ext_row_t *, s5gpu_site_cell_t *, s5gpu_site_score_t *, int32_t *)'
                   ' = s5gpu_sites_add_batch;\n'
                   'int (*h)(void *, void *) = s5gpu_sites_close;\n'
                   'printf("%d %zu %zu\\n", a && b && c && d && e && f && g && h, sizeof(s5gpu_site_cell_t), sizeof(s5gpu_site_score_t));return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == ["1", "16", "16"]
    # the tool: without arguments its usage (exit 2); with files that do not exist it gets as far as opening the reference
    p = subprocess.run([sites.S5SITES], capture_output=True)
    assert p.returncode == 2 and b"usage: s5sites" in p.stderr and b"--sites" in p.stderr and b"--control" in p.stderr and p.stdout == b""
    none = [str(tmp_path / "none.txt"), str(tmp_path / "a.blow5")]
    p = subprocess.run([sites.S5SITES, "--q0", "-200", "--shift", "3", "--tile", "64", "--band", "128", "--sites", str(tmp_path / "s.txt")] + none, capture_output=True)
    assert p.returncode == 2 and b"usage" not in p.stderr and b"cannot open" in p.stderr, p.stderr
    for args in (["--shift", "11"], ["--q0", "32768"], ["--tile", "100"], ["--band", "100"], ["--bogus"], ["--sites"]):
        p = subprocess.run([sites.S5SITES] + args + none, capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr, (args, p.stderr)
    p = subprocess.run([sites.S5SITES] + none, capture_output=True)                                 # no --sites
    assert p.returncode == 2 and b"usage" in p.stderr
    # the site file: a column at or beyond the reference's end, and a line that is no column, are refused before a device is needed
    ref = tmp_path / "ref.txt"
    ref.write_text("".join("%d\n" % v for v in range(400, 410)))
    for text, why in (("3\n10\n", b"position 10"), ("3\nx\n", b"is not a position"), ("-1\n", b"is not a position"), ("# none\n\n", b"no position")):
        (tmp_path / "s.txt").write_text(text)
        p = subprocess.run([sites.S5SITES, "--sites", str(tmp_path / "s.txt"), str(ref), none[1]], capture_output=True)
        assert p.returncode == 2 and why in p.stderr and b"usage" not in p.stderr, (text, p.stderr)


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3): the pointers are never dereferenced on the host, so made-up aligned addresses serve"""
    from slow5tools_amd import _lib, sites

    L = _lib.lib()
    P = 1 << 20
    need = L.s5gpu_pileup_long_work_bytes(4, 1000)

    def cells(n=4, q=P, first=P, ql=P, total=1000, R=100, lo=P, hi=P, st=P, s=P, M=3, work=P, wb=need, out=P, v=None):
        return L.s5gpu_site_cells_long_dev(n, q, first, ql, total, R, lo, hi, st, s, M, work, wb, out, v, None)
    assert cells(R=0) == -1 and cells(R=(1 << 22) + 1) == -1 and cells(total=(1 << 40) + 1) == -1
    for name in ("q", "first", "ql", "lo", "hi", "st", "work", "s", "out"):
        assert cells(**{name: None}) == -1, name
    assert cells(q=P + 1) == -1 and cells(first=P + 4) == -1 and cells(ql=P + 2) == -1 and cells(lo=P + 2) == -1 and cells(hi=P + 1) == -1
    assert cells(st=P + 2) == -1 and cells(work=P + 8) == -1 and cells(out=P + 8) == -1 and cells(s=P + 2) == -1 and cells(v=P + 2) == -1
    assert cells(M=0) == -1 and cells(M=65537) == -1 and cells(n=2049, M=65536) == -1 and cells(n=(1 << 27) + 1, M=1) == -1
    assert cells(wb=need - 1) == -3 and cells(wb=0) == -3
    assert cells(n=0) == 0 and cells(n=0, q=None, first=None, lo=None, work=None, wb=0) == 0        # nothing to do: nothing is launched
    assert cells(n=0, out=None) == -1 and cells(n=0, s=None) == -1 and cells(n=0, R=0) == -1 and cells(n=0, M=0) == -1

    def score(c=P, n=4, s=P, M=3, hist=P, R=100, out=P):
        return L.s5gpu_site_score_dev(c, n, s, M, hist, R, out, None)
    for kw in (dict(c=None), dict(s=None), dict(hist=None), dict(out=None), dict(c=P + 8), dict(s=P + 2), dict(hist=P + 8), dict(out=P + 8), dict(R=0),
               dict(R=(1 << 22) + 1), dict(M=0), dict(M=65537), dict(n=2049, M=65536)):
        assert score(**kw) == -1, kw
    assert score(n=0) == 0
    vp = C.c_void_p
    h_ref = np.zeros(100, dtype=np.int16)

    def opened(mp=(0, 64, 10, 32.0, 127, 1), bp=(0, 10, 1 << 20, 256, 512, 127, 32.0), ev=(3, 6, 1.4, 9.0, 0.2), R=100, ref=True, bp_null=False, q0=-128, shift=2,
               s=(3, 50, 99), s_null=False, M=None):
        e, m, b = _lib.EventParams(*ev), _lib.MapParams(*mp), _lib.BandParams(*bp)
        ref_p = (np.zeros(R, dtype=np.int16) if R > 100 else h_ref).ctypes.data_as(vp) if ref else None
        sa = np.array(s, dtype=np.uint32)
        h = L.s5gpu_sites_open(C.byref(e), C.byref(m), None if bp_null else C.byref(b), 0, ref_p, R, None if s_null else sa.ctypes.data_as(vp),
                               len(sa) if M is None else M, q0, shift)
        return h, L.s5gpu_last_error()
    for kw in (dict(bp_null=True), dict(bp=(0, 10, 1 << 20, 100, 512, 127, 32.0)), dict(mp=(0, 0, 1, 32.0, 127, 1)), dict(R=0), dict(R=(1 << 22) + 1), dict(ref=False),
               dict(q0=32768), dict(q0=-32769), dict(shift=11), dict(s=(50, 3, 99)), dict(s=(3, 3, 99)), dict(s=(3, 50, 100)), dict(s_null=True), dict(M=0),
               dict(M=65537)):
        h, why = opened(**kw)
        assert h is None and why.startswith(b"s5gpu_sites_open:") and b"device" not in why, (kw, why)
    assert L.s5gpu_sites_add_batch(None, 0, None, None, 1, 1, None, None, None, None) == -1
    assert L.s5gpu_sites_add_control(None, 0, None, None, 1, 1, None) == -1 and L.s5gpu_sites_set_control(None, None) == -1
    assert L.s5gpu_sites_set_refine(None, None) == -1 and L.s5gpu_sites_close(None, None) == 0
    # the module: an unsorted list, a duplicated one, one with a column at R, an empty one
    for bad in ([5, 3], [3, 3], [3, 100], [-1, 3], [], [[1, 2]], [1.5]):
        with pytest.raises(ValueError):
            sites.check_sites(bad, 100)
    assert sites.check_sites([0, 99], 100).tolist() == [0, 99] and sites.check_sites(np.arange(65536), 1 << 20).dtype == np.uint32
    with pytest.raises(ValueError):
        sites.check_sites(np.arange(65537), 1 << 20)
    for bad in ([5, 3], [3, 3]):
        with pytest.raises(ValueError):
            sites.Sites(h_ref, bad)
        with pytest.raises(ValueError):
            sites.file_sites("none.blow5", "none.txt", bad)
    with pytest.raises(ValueError):
        sites.Sites(h_ref, [3, 100])
    assert L.s5gpu_set_option(b"site_passes", 0) == -1 and L.s5gpu_set_option(b"site_passes", 8) == -1 and L.s5gpu_set_option(b"site_passes", 7) == 0


def test_the_restatements():
    # hand-made: two reads on 4 columns; read 0 rows (0..1), (1..1), (2..3); read 1 rows (1..1), (1..2)
    q = np.array([-128, -125, 0, 127, 200], dtype=np.int16)
    lo, hi = np.array([0, 1, 2, 1, 1], dtype=np.int32), np.array([1, 1, 3, 1, 2], dtype=np.int32)
    case = LongCase(q, [0, 3, 5], [3, 2], [0, 0, 0, 0], lo, hi)
    got = cells_ref(case, [0, 1, 2, 3])
    assert got.tolist() == [[(-128, 1, 0), (0, 0, ROW_NONE)], [(-253, 2, 0), (327, 2, 0)], [(0, 1, 2), (200, 1, 1)], [(0, 1, 2), (0, 0, ROW_NONE)]]
    assert verdicts_ref(case).tolist() == [0, 0]
    case.status[1] = 5
    assert cells_ref(case, [1])["cells"].tolist() == [[2, 0]] and verdicts_ref(case).tolist() == [0, 1]
    # the level: the mean rounded half up, the floor for negatives too
    assert [sr.level_ref(s, c) for s, c in ((-1, 2), (-3, 2), (1, 2), (3, 2), (-7, 3), (-8, 3), (7, 3), (8, 3), (-65536, 2), (65534, 2), (-65535, 2))] == [
        0, -1, 1, 2, -2, -3, 2, 3, -32768, 32767, -32767]
    # the score: column 0 of the control holds 1, 2, 3 cells in bins 30, 32, 34 (levels -8 .. -5, 0 .. 3, 8 .. 11 at the default bins)
    counts = np.zeros((2, BINS), np.int64)
    counts[0, [30, 32, 34]] = [1, 2, 3]
    cells = np.zeros((2, 4), dtype=SITE_CELL)
    cells[:] = [[(0, 1, 0), (-40, 2, 3), (9, 1, 0), (0, 0, ROW_NONE)]] * 2
    rows = score_ref(cells, [0, 1], counts, Q0, SHIFT)
    assert rows[0].tolist() == [(0, 0, 3, 5, 6), (-20, 0, 0, 6, 6), (9, 0, 6, 3, 6), (0, 1, 0, 0, 6)]
    assert rows[1].tolist() == [(0, 2, 0, 0, 0), (-20, 2, 0, 0, 0), (9, 2, 0, 0, 0), (0, 3, 0, 0, 0)]
    assert (score_ref(cells, [0, 1], counts, Q0, SHIFT, R=3)["flags"] == 128).all() and (score_ref(cells, [0, 1], counts, Q0, SHIFT, bins=32)["flags"] == 128).all()
    big = np.full((1, BINS), 2 ** 32 - 1, np.int64)
    assert score_ref(cells[:1], [0], big, Q0, SHIFT)[0, 0].tolist() == (0, 0, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)
    # every case and every site list: the invariants against hist_ref and pileup_long_ref are asserted inside cells_ref
    seen = set()
    for name in hist_cases():
        for label, s in site_lists(name).items():
            assert wanted(name, label).shape == (len(s), hist_cases()[name][0].n)
            seen.add(label)
    assert seen == {"column 0", "column R - 1", "spread", "left of every path", "right of every path", "every column", "inside the 70-wide row",
                    "the 64 piled reads", "a stay across a seam", "the 300-wide rows", "a column no read crosses"}
    two = wanted("seams", "a stay across a seam")                           # rows 63 and 64 (127 and 128) of read 1: two segments, one entry
    assert two["cells"][:, 1].min() >= 2 and two["row0"][0, 1] <= 63 and two["row0"][1, 1] <= 127
    assert wanted("edges R=300 q0=-128 shift=2", "the 64 piled reads")["cells"][:, 3:67].tolist() == [[1] * 64] * 3
    for c in sr.score_hand_cases():
        assert score_ref(*c[1:]).shape == c[1].shape


SITES_HOST = r'''
// The code of sites_dev.h on the CPU, with plain adds in place of the atomics.
// mode 0: what k_pileup_long_plan, _check, k_site_fill and k_site_cells do with it, every array allocated at exactly its size, the segments
// visited in a shuffled order, each resolved by seg_item of ragged_dev.h.
//   in.bin: 0, n, R, S, M, seed (uint32), total_rows (uint64), then first, qlen, status, queries, lo, hi, sites; out.bin: the matrix, the verdicts.
// mode 1: what k_site_score does with it, a column at a time.
//   in.bin: 1, n, R, M, the histogram's columns, 0 (uint32), 0 (uint64), then sites, the histogram, the matrix; out.bin: the rows.
#define S5_PILEUP_HOST
#include "sites_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
using namespace pilek;
struct HostOps {
    static void add64(uint64_t *p, uint64_t v) { *p += v; }
    static void add32(uint32_t *p, uint32_t v) { *p += v; }
    static void min32(uint32_t *p, uint32_t v) { if (v < *p) *p = v; }
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

static int score(FILE *f, FILE *o, const uint32_t *h) {
    const uint32_t n = h[1], R = h[2], M = h[3], hist_cols = h[4];
    uint32_t *sites = get<uint32_t>(f, M);
    uint32_t *hist = get<uint32_t>(f, HIST_HEAD_WORDS + (size_t)hist_cols * HIST_BINS);
    s5gpu_site_cell_t *cells = get<s5gpu_site_cell_t>(f, (size_t)M * n);
    s5gpu_site_score_t *out = (s5gpu_site_score_t *)malloc((size_t)M * n ? (size_t)M * n * sizeof *out : 1);
    const bool head = site_head_ok(hist, R);
    const int32_t q0 = (int32_t)hist[9];
    const uint32_t shift = hist[10];
    for (uint32_t t = 0; t < M; t++) {
        const bool col = sites[t] < R;
        uint64_t cum[HIST_BINS], run = 0;
        for (uint32_t b = 0; b < HIST_BINS; b++) { run += head && col ? hist[HIST_HEAD_WORDS + (size_t)sites[t] * HIST_BINS + b] : 0u; cum[b] = run; }
        for (uint32_t k = 0; k < n; k++) {
            const s5gpu_site_cell_t e = cells[(size_t)t * n + k];
            int16_t level;
            const uint32_t b = site_level_bin(e, q0, shift, &level);
            if (b >= HIST_BINS) return 3;
            out[(size_t)t * n + k] = head ? site_score_row(e, level, cum[b], b ? cum[b - 1] : 0u, run, col ? 0u : S5GPU_SITE_COLUMN) : site_score_head();
        }
    }
    fwrite(out, sizeof *out, (size_t)M * n, o);
    free(sites); free(hist); free(cells); free(out);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t h[6];
    uint64_t total_rows;
    if (!f || !o || fread(h, 4, 6, f) != 6 || fread(&total_rows, 8, 1, f) != 1) return 1;
    if (h[0] == 1) {
        const int rc = score(f, o, h);
        fclose(f);
        return rc ? rc : fclose(o) == 0 ? 0 : 1;
    }
    const uint32_t n = h[1], R = h[2], S = h[3], M = h[4];
    g_rand = h[5];
    uint64_t *first = get<uint64_t>(f, (size_t)n + 1);
    uint32_t *qlen = get<uint32_t>(f, n);
    int32_t *status = get<int32_t>(f, n);
    int16_t *q = get<int16_t>(f, total_rows);
    int32_t *lo = get<int32_t>(f, total_rows), *hi = get<int32_t>(f, total_rows);
    uint32_t *sites = get<uint32_t>(f, M);
    const PileLongArgs A = {n, q, first, qlen, total_rows, nullptr, R, lo, hi, status, nullptr, 0u, nullptr, nullptr};
    uint32_t *verdict = (uint32_t *)malloc(n ? 4ull * n : 1);
    uint64_t *P = (uint64_t *)malloc(8ull * (n + 1ull));
    const LongPtrs L = {verdict, P, nullptr, nullptr, nullptr, 0};
    P[0] = 0;
    for (uint32_t k = 0; k < n; k++) {
        verdict[k] = long_verdict(first[k], first[k + 1], qlen[k], status[k], total_rows, 0u);
        P[k + 1] = P[k] + (verdict[k] == V_USED ? segs_of(qlen[k], S) : 0u);
    }
    const uint64_t total = P[n];
    uint64_t *list = (uint64_t *)malloc(total ? 8 * total : 1);
    for (uint64_t g = 0; g < total; g++) list[g] = g;
    shuffle(list, total);
    for (uint64_t x = 0; x < total; x++) {                                  // every segment through seg_item, the kernels' resolver
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, false, list[x], &g)) return 4;
        if (!seg_rows_ok(g.r0, g.r1, 0, 1, lo + first[g.k], hi + first[g.k], R)) verdict[g.k] |= V_BAD;
    }
    shuffle(list, total);
    // the matrix at exactly M n entries: the fill, then the cells
    const size_t entries = (size_t)M * n;
    s5gpu_site_cell_t *out = (s5gpu_site_cell_t *)malloc(entries ? entries * sizeof *out : 1);
    for (size_t e = 0; e < entries; e++) { out[e].sum_q = 0; out[e].cells = 0u; out[e].row0 = SITE_ROW_NONE; }
    for (uint64_t x = 0; x < total; x++) {
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, false, list[x], &g)) return 4;
        if (verdict[g.k] != V_USED) continue;
        site_seg_cells<HostOps>(g.r0, g.r1, 0, 1, lo + first[g.k], hi + first[g.k], q + first[g.k], sites, M, g.k, n, out);
    }
    for (uint32_t k = 0; k < n; k++) verdict[k] = (verdict[k] & V_SKIPPED) ? 1u : (verdict[k] & V_BAD) ? 2u : 0u;
    fwrite(out, sizeof *out, entries, o);
    fwrite(verdict, 4, n, o);
    free(out); free(list); free(P); free(verdict); free(first); free(qlen); free(status); free(q); free(lo); free(hi); free(sites);
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _run_cells_host(exe, tmp_path, case, sites, S=64, seed=1):
    s = np.asarray(sites, dtype=np.uint32)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<6IQ", 0, case.n, case.R, S, len(s), seed, case.total))
        for a in (case.first, case.qlen, case.status, case.q, case.lo, case.hi, s):
            fh.write(a.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = (tmp_path / "out.bin").read_bytes()
    nb = 16 * len(s) * case.n
    assert len(raw) == nb + 4 * case.n
    return np.frombuffer(raw[:nb], dtype=SITE_CELL).reshape(len(s), case.n), np.frombuffer(raw[nb:], dtype="<u4")


def _hist_of(counts, q0, shift, bins=BINS):
    counts = np.asarray(counts)
    head = np.zeros(1, dtype=HIST_HEAD)
    head[0] = (int(counts.astype(object).sum()) % 2 ** 64, 0, 0, 0, len(counts), q0, shift, bins, (0, 0))
    return hist_bytes_of((head[0], counts))


def _run_score_host(exe, tmp_path, cells, sites, counts, q0, shift, R, bins):
    s = np.asarray(sites, dtype=np.uint32)
    M, n = cells.shape
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<6IQ", 1, n, R, M, len(counts), 0, 0) + s.tobytes() + _hist_of(counts, q0, shift, bins) + np.ascontiguousarray(cells).tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=SITE_SCORE).reshape(M, n)


def run_sites_header_on_the_cpu(tmp_path, extra=()):
    exe = host_build(tmp_path, "sites_host", SITES_HOST, ["-O1", "-g", "-std=c++17", "-Wall"], extra, api=True)
    for name, (case, q0, shift) in hist_cases().items():
        v = verdicts_ref(case)
        for label, s in site_lists(name).items():
            for S, seed in ((64, 1), (256, 2)):
                got, verdict = _run_cells_host(exe, tmp_path, case, s, S, seed)
                assert got.tobytes() == wanted(name, label).tobytes(), (name, label, S, _explain(got, wanted(name, label)))
                assert verdict.tolist() == v.tolist(), (name, label, S)
    for c in sr.score_hand_cases():
        got, want = _run_score_host(exe, tmp_path, *c[1:]), score_ref(*c[1:])
        assert got.tobytes() == want.tobytes(), (c[0], _explain(got, want))


def test_the_header_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """site_lower, site_range, site_cell_add, site_row_cells, site_seg_cells, site_level, site_level_bin, site_score_row and site_head_ok of
    sites_dev.h as g++ compiles them, over the case list and its site lists at segments of 64 and 256, and over the hand-made controls"""
    run_sites_header_on_the_cpu(tmp_path)


def test_the_header_code_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: every array is allocated at exactly its size"""
    run_sites_header_on_the_cpu(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def test_the_planted_case_at_the_query_level():
    """the control is reads 0 .. 7 of side 0; every one of the sixteen scored reads has a cell at all ten sites, and every side-1 read has
    strictly more sites where one tail of the control is empty than every held-out side-0 read"""
    scores, cells, labels = sr.planted_scores()
    own, other = sr.planted_condition(scores, cells, labels)
    print("planted: zero-tail sites of the held-out side-0 reads", own, "of the side-1 reads", other)


# ---------------------------------------------------------------------------------------------------------------- gpu

def _options(env, seg=64, grid=DEFAULT_GRID):
    for key, v in ((b"pileup_long_seg", seg), (b"pileup_long_grid", grid)):
        env.lib.check(env.L.s5gpu_set_option(key, v), key.decode())


class Uploaded:
    """a case's inputs on the device, uploaded once"""

    def __init__(self, env, case):
        self.env, self.case = env, case
        self.host = [case.q, case.first.view(np.int64), case.qlen.view(np.int32), case.lo, case.hi, case.status]
        self.dev = [env.torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in self.host]
        self.need = env.L.s5gpu_pileup_long_work_bytes(case.n, case.total)

    def unchanged(self):
        for t, a in zip(self.dev, self.host):
            assert np.array_equal(t.cpu().numpy(), a), "an input was written"


def _cells(env, up, sites, stream=None, sync=True, short=0, want_rc=0):
    """THE way into s5gpu_site_cells_long_dev here: the matrix, the verdicts and a work area of exactly the size asked for between guards of
    0x5A, the call made on `stream`, and afterwards the guards checked.  short: the bytes the call is told are missing."""
    torch, case = env.torch, up.case
    s = torch.from_numpy(np.asarray(sites, dtype=np.uint32).view(np.int32).copy()).to("cuda")
    M, n = len(sites), case.n
    out = torch.full((16 * M * n + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    ver = torch.full((4 * n + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    work = torch.full((up.need + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if t.numel() else None for t in up.dev]
    rc = env.L.s5gpu_site_cells_long_dev(n, ptr[0], ptr[1], ptr[2], case.total, case.R, ptr[3], ptr[4], ptr[5], s.data_ptr(), M, work.data_ptr() + 64, up.need - short,
                                         out.data_ptr() + 64, ver.data_ptr() + 64, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == want_rc, (rc, env.L.s5gpu_last_error())

    def check():
        o, v, w = out.cpu().numpy(), ver.cpu().numpy(), work.cpu().numpy()
        for a, what in ((o, "matrix"), (v, "verdicts"), (w, "work area")):
            assert (a[:64] == 0x5A).all() and (a[-64:] == 0x5A).all(), "a guard of the %s was written" % what
        if want_rc != 0:
            assert (o == 0x5A).all() and (v == 0x5A).all() and (w == 0x5A).all(), "a call that was refused wrote"
            return None, None
        assert np.array_equal(s.cpu().numpy().view(np.uint32), np.asarray(sites, dtype=np.uint32)), "the site list was written"
        return o[64:-64].view(SITE_CELL).reshape(M, n), v[64:-64].view("<u4")
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hist_cases()))
def test_the_case_list_is_exact(gpu, name):
    case = hist_cases()[name][0]
    up = Uploaded(gpu, case)
    v = verdicts_ref(case)
    _options(gpu)
    try:
        for label, s in site_lists(name).items():
            got, verdict = _cells(gpu, up, s)
            want = wanted(name, label)
            assert got.tobytes() == want.tobytes(), (label, _explain(got, want))
            assert verdict.tolist() == v.tolist(), label
        up.unchanged()
    finally:
        _options(gpu, seg=DEFAULT_SEG)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges R=300 q0=-128 shift=2", "edges R=65 q0=0 shift=0", "seams", "piling"])
def test_the_options_do_not_change_a_byte(gpu, name):
    up = Uploaded(gpu, hist_cases()[name][0])
    try:
        for seg, grid in SETTINGS:
            _options(gpu, seg, grid)
            for label, s in site_lists(name).items():
                got, _ = _cells(gpu, up, s)
                want = wanted(name, label)
                assert got.tobytes() == want.tobytes(), (seg, grid, label, _explain(got, want))
    finally:
        _options(gpu, seg=DEFAULT_SEG)


@pytest.mark.gpu
def test_two_calls_on_two_streams_and_a_short_work_area(gpu):
    torch = gpu.torch
    case = mixed_case(129, 200)
    a, b = relay(case.part(0, 90)), relay(case.part(90, 200))
    sites = sorted(set(int(x) for x in np.linspace(0, case.R - 1, 40)))
    ua, ub = Uploaded(gpu, a), Uploaded(gpu, b)
    _options(gpu)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        checks = [_cells(gpu, ua, sites, stream=s1, sync=False), _cells(gpu, ub, sites, stream=s2, sync=False)]
        torch.cuda.synchronize()
        for f, c in zip(checks, (a, b)):
            got, verdict = f()
            want = cells_ref(c, sites)
            assert got.tobytes() == want.tobytes(), _explain(got, want)
            assert verdict.tolist() == verdicts_ref(c).tolist() and want["cells"].sum() > 0
        # a work area one byte short: S5GPU_ERR_NOMEM, and neither the matrix, the verdicts nor the work area is touched
        _cells(gpu, ua, sites, short=1, want_rc=-3)
        ua.unchanged()
        ub.unchanged()
    finally:
        _options(gpu, seg=DEFAULT_SEG)


@pytest.mark.gpu
def test_a_fixed_pitch_batch_equals_the_ragged_call(gpu):
    torch, st = gpu.torch, gpu.sites
    case = mixed_case(129, 200)
    ragged = relay(case, seed=3)
    sites = sorted(set(int(x) for x in np.linspace(0, case.R - 1, 40)))
    want = cells_ref(ragged, sites)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    cells, verdict = st.cells_dev(dev(case.qm), dev(case.qlen.view(np.int32)), dev(case.lo), dev(case.hi), dev(case.status), sites, case.R)
    got = st.cells_to_host(cells)
    assert got.tobytes() == want.tobytes(), _explain(got, want)
    assert verdict.cpu().numpy().tolist() == verdicts_ref(ragged).tolist()
    got, _ = _cells(gpu, Uploaded(gpu, relay(case)), sites)
    assert got.tobytes() == want.tobytes(), _explain(got, want)
    with pytest.raises(ValueError):
        st.cells_dev(dev(case.qm), dev(case.qlen.view(np.int32)), dev(case.lo), dev(case.hi), dev(case.status), [5, 3], case.R)
    # an empty batch: a matrix of no reads
    none = long_cases()["empty batch"]
    cells, verdict = st.cells_long_dev(dev(none.q), dev(none.first.view(np.int64)), dev(none.qlen.view(np.int32)), dev(none.lo), dev(none.hi), dev(none.status), [0, 2], none.R)
    assert tuple(cells.shape) == (2, 0, 2) and st.cells_to_host(cells).shape == (2, 0) and verdict.numel() == 0


def _score(env, cells, sites, counts, q0, shift, R, bins=BINS):
    """s5gpu_site_score_dev on an uploaded matrix, list and histogram; the rows between guards"""
    torch = env.torch
    M, n = cells.shape
    c = torch.from_numpy(np.frombuffer(np.ascontiguousarray(cells).tobytes(), dtype=np.uint8).copy()).to("cuda")
    s = torch.from_numpy(np.asarray(sites, dtype=np.uint32).view(np.int32).copy()).to("cuda")
    h = torch.from_numpy(np.frombuffer(_hist_of(counts, q0, shift, bins), dtype=np.uint8).copy()).to("cuda")
    out = torch.full((16 * M * n + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    env.lib.check(env.L.s5gpu_site_score_dev(c.data_ptr(), n, s.data_ptr(), M, h.data_ptr(), R, out.data_ptr() + 64, None), "s5gpu_site_score_dev")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:64] == 0x5A).all() and (o[-64:] == 0x5A).all(), "a guard of the rows was written"
    return o[64:-64].view(SITE_SCORE).reshape(M, n)


@pytest.mark.gpu
def test_the_score_on_hand_made_controls(gpu):
    for c in sr.score_hand_cases():
        got, want = _score(gpu, *c[1:]), score_ref(*c[1:])
        assert got.tobytes() == want.tobytes(), (c[0], _explain(got, want))
    # the module's wrapper on one of them
    label, cells, sites, counts, q0, shift, R, bins = sr.score_hand_cases()[-1]
    t = gpu.torch.from_numpy(cells.view("<i8").reshape(cells.shape + (2,)).copy()).to("cuda")
    h = gpu.torch.from_numpy(np.frombuffer(_hist_of(counts, q0, shift), dtype=np.uint8).copy()).to("cuda")
    got = gpu.sites.scores_to_host(gpu.sites.score_dev(t, sites, h))
    assert got.tobytes() == score_ref(cells, sites, counts, q0, shift).tobytes()
    tail = gpu.sites.tail(got)
    assert np.isnan(tail[got["flags"] != 0]).all() and (tail[got["flags"] == 0] <= 1.0).all() and (tail[got["flags"] == 0] >= 0.0).all()


@pytest.mark.gpu
def test_the_planted_case_through_the_device(gpu):
    """extend.band_dev -> hist_accum_long_dev (reads 0 .. 7 of side 0) and cells_long_dev -> score_dev (the other sixteen): the restatement fed
    with the device's lo / hi, byte for byte, and the planted condition on the device's rows"""
    torch, ex, ct, st = gpu.torch, gpu.extend, gpu.contrast, gpu.sites
    ref, sides = cr.planted()
    p = ex.BandParams(0, 1, 1 << 20, 64, 128)

    def dev(a, dtype=None):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")

    def run(reads):
        Q = [len(q) for q, _ in reads]
        first = np.concatenate(([0], np.cumsum(Q))).astype(np.int64)
        q, ql, s0 = dev(np.concatenate([q for q, _ in reads])), dev(Q, np.int32), dev(np.zeros(len(Q)), np.int32)
        rows, lo, hi = ex.band_dev(q, dev(first), ql, dev(ref), dev([a for _, a in reads], np.int32), s0, p, None)
        status = (rows[:, 3] >> 32).to(torch.int32)
        assert status.cpu().numpy().tolist() == [0] * len(Q)
        h_lo, h_hi = lo.cpu().numpy(), hi.cpu().numpy()
        return (q, dev(first), ql, lo, hi, status), [(h_lo[first[k]:first[k + 1]], h_hi[first[k]:first[k + 1]]) for k in range(len(Q))]
    ctl, ctl_paths = run(sides[0][:8])
    held, held_paths = run(sides[0][8:] + sides[1])
    hist = ct.hist_accum_long_dev(*ctl, ct.new_hist(len(ref)))
    cells, verdict = st.cells_long_dev(*held, sr.PLANTED_SITES, len(ref))
    scores = st.scores_to_host(st.score_dev(cells, sr.PLANTED_SITES, hist))
    cells = st.cells_to_host(cells)
    paths = [list(ctl_paths) + list(held_paths[:4]), list(held_paths[4:])]
    want_scores, want_cells, labels = sr.planted_scores(paths)
    assert cells.tobytes() == want_cells.tobytes(), _explain(cells, want_cells)
    assert scores.tobytes() == want_scores.tobytes(), _explain(scores, want_scores)
    assert verdict.cpu().numpy().tolist() == [0] * 16
    sr.planted_condition(scores, cells, labels)


FILE_SITES = list(range(60, 3500, 137))


@pytest.fixture(scope="module")
def files(gpu):
    """two small synthetic files, made as test_contrast's (one read a side too short for a query): file 0 is the control, file 1 is scored"""
    rng = np.random.default_rng(4025)
    levels = rng.normal(500.0, 110.0, 3500).astype(np.float32)
    env = type("Files", (), {})()
    env.levels, env.ref = levels, quant_ref(levels)
    env.recs = [[record(10 * s + i, levels_signal(n, rng)) for i, n in enumerate(lengths)] for s, lengths in enumerate(([30000, 100, 26000, 28000], [27000, 31000, 100]))]
    env.ids = [[ob.synth_read_id(10 * s + i) for i in range(len(r))] for s, r in enumerate(env.recs)]
    env.ids = [[i if isinstance(i, bytes) else i.encode() for i in side] for side in env.ids]
    env.kw = dict(skip=2, qmax=100, qmin=20, tile_rows=64, band=128)
    return env


def _chain_case(ref, x):
    rows = x.rows.cpu().numpy().view(EXT_ROW).reshape(-1)
    return LongCase(x.queries.cpu().numpy(), x.first.cpu().numpy().astype(np.uint64), x.qlen.cpu().numpy(), ref, x.lo.cpu().numpy(), x.hi.cpu().numpy(), rows["status"])


def _whole(gpu, files, refine):
    """sites_whole_dev on the two files, held against the restatement fed with the chain's own paths"""
    st, ct = gpu.sites, gpu.contrast
    dec = [gpu.press.decode_to_device(r) for r in files.recs]
    cells, verdict, scores, hist, x = st.sites_whole_dev(dec[1], files.ref, FILE_SITES, control=dec[0], refine=refine, **files.kw)
    cells, scores, hist = st.cells_to_host(cells), st.scores_to_host(scores), ct.hist_to_host(hist)
    case = _chain_case(files.ref, x)
    want = cells_ref(case, FILE_SITES)
    assert cells.tobytes() == want.tobytes(), _explain(cells, want)
    assert verdict.cpu().numpy().tolist() == verdicts_ref(case).tolist() == [0, 0, 1]
    want = score_ref(cells, FILE_SITES, hist[1].astype(np.int64), Q0, SHIFT)
    assert scores.tobytes() == want.tobytes(), _explain(scores, want)
    assert (cells["cells"][:, :2] > 0).sum() > 20 and (scores["n"] > 0).sum() > 20 and hist[0]["reads_used"] == 3 and hist[0]["reads_skipped"] == 1
    # without a control: the same cells, no scores; with the histogram as a tensor: the same scores
    c2, _, s2, h2, _ = st.sites_whole_dev(dec[1], files.ref, FILE_SITES, refine=refine, **files.kw)
    assert s2 is None and h2 is None and st.cells_to_host(c2).tobytes() == cells.tobytes()
    return cells, scores, hist


def _lines(files, cells, scores, control=True):
    """the tool's lines, composed from the matrix and its rows"""
    out = []
    for k, rid in enumerate(files.ids[1]):
        for t, s in enumerate(FILE_SITES):
            c, r = cells[t, k], scores[t, k]
            if c["cells"] == 0:
                continue
            line = b"%s\t%d\t%d\t%d\t%d" % (rid, s, c["cells"], sr.level_ref(c["sum_q"], c["cells"]), files.kw["skip"] + int(c["row0"]))
            if not control:
                line += b"\t.\t.\t.\t."
            elif r["n"] == 0:
                line += b"\t%d\t%d\t%d\t." % (r["below"], r["above"], r["n"])
            else:
                line += b"\t%d\t%d\t%d\t%s" % (r["below"], r["above"], r["n"], b"%.6g" % min(1.0, 2.0 * float(min(r["below"], r["above"])) / float(r["n"])))
            out.append(line + b"\n")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [None, True], ids=["plain", "refine"])
def test_the_chain_the_handle_and_the_tool(gpu, files, refine, tmp_path):
    st = gpu.sites
    cells, scores, hist = _whole(gpu, files, refine)
    # the handle: the control added a batch at a time, the file in one batch and in two
    with st.Sites(files.ref, FILE_SITES, refine=refine, **files.kw) as h:
        for part in (files.recs[0][:3], files.recs[0][3:]):
            rc, status = h.add_control(part)
            assert rc == 0 and len(status) == len(part)
        rc, rows, c1, s1, status = h.add(files.recs[1])
        assert rc == 0 and c1.tobytes() == cells.tobytes() and s1.tobytes() == scores.tobytes(), (_explain(c1, cells), _explain(s1, scores))
        assert status[2] != 0 and rows["qlen"][2] == 0 and (rows["qlen"][:2] > 2000).all()
        parts = [h.add(files.recs[1][:1]), h.add(files.recs[1][1:], scores=False)]
        assert np.concatenate([p[2] for p in parts], axis=1).tobytes() == cells.tobytes() and parts[0][3].tobytes() == scores[:, :1].tobytes() and parts[1][3] is None
        got = h.close()
    assert hist_bytes_of(got) == hist_bytes_of(hist)
    # ... against set_control of the same histogram; a histogram of another shift is refused
    with st.Sites(files.ref, FILE_SITES, refine=refine, **files.kw) as h:
        other = (hist[0].copy(), hist[1])
        other[0]["shift"] = 3
        with pytest.raises(gpu.lib.S5GpuError, match="rc=-1"):
            h.set_control(other)
        h.set_control(hist)
        rc, _, c1, s1, _ = h.add(files.recs[1])
        assert c1.tobytes() == cells.tobytes() and s1.tobytes() == scores.tobytes()
        # a corrupt record: -5, its entries empty and scored as such, the rest valid, the handle usable
        recs = list(files.recs[1])
        bad = bytearray(recs[0])
        bad[-1] ^= 0x5A                                                    # the Adler-32 of the zlib stream
        recs[0] = bytes(bad)
        with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
            h.add(recs)
        rc, rows, c1, s1, status = h.add(recs, raise_on_error=False)
        assert rc == -5 and status[0] != 0 and rows["qlen"][0] == 0
        assert (c1["cells"][:, 0] == 0).all() and (c1["row0"][:, 0] == ROW_NONE).all() and c1[:, 1:].tobytes() == cells[:, 1:].tobytes()
        assert s1[:, 0].tobytes() == scores[:, 2].tobytes() and s1[:, 1:].tobytes() == scores[:, 1:].tobytes() and (s1["flags"][:, 0] & 1).all()
        rc, _, c1, _, _ = h.add(files.recs[1])
        assert rc == 0 and c1.tobytes() == cells.tobytes()
        assert hist_bytes_of(h.close()) == hist_bytes_of(hist)
    # the tool and file_sites
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("".join("%.9g\n" % v for v in files.levels))
    for s, name in enumerate(("ctl.blow5", "reads.blow5")):
        synth_file(tmp_path / name, files.recs[s])
    sites_txt = tmp_path / "sites.txt"
    sites_txt.write_text("# unsorted, one twice\n" + "".join("%d\n" % v for v in FILE_SITES[::-1] + FILE_SITES[:1]))
    kw = files.kw
    args = ["--skip", str(kw["skip"]), "--events", str(kw["qmax"]), "--min-events", str(kw["qmin"]), "--tile", str(kw["tile_rows"]), "--band", str(kw["band"])]
    args += ["--refine"] if refine else []
    tail = ["--sites", str(sites_txt), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([st.S5SITES, "-K", "2", "--control", str(tmp_path / "ctl.blow5")] + args + tail, capture_output=True, timeout=120)
    want = _lines(files, cells, scores)
    assert p.returncode == 0 and b"ctl.blow5: reads used 3, skipped 1, bad 0" in p.stderr and b"reads 3, with a line 2" in p.stderr, p.stderr
    assert p.stdout == b"".join(want) and len(want) > 20
    p = subprocess.run([st.S5SITES, "-K", "2"] + args + tail, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(_lines(files, cells, scores, control=False)), p.stderr
    t = st.file_sites(str(tmp_path / "reads.blow5"), str(ref_txt), FILE_SITES, control=str(tmp_path / "ctl.blow5"), refine=refine,
                      batch=2, tile_rows=kw["tile_rows"], band=kw["band"], skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"])
    at = [(k, t_) for k in range(3) for t_ in range(len(FILE_SITES)) if cells["cells"][t_, k]]
    assert t["read_id"].tolist() == [files.ids[1][k].decode() for k, _ in at] and t["ref_pos"].tolist() == [FILE_SITES[t_] for _, t_ in at]
    assert t["cells"].tolist() == [int(cells["cells"][t_, k]) for k, t_ in at] and t["level"].tolist() == [int(scores["level"][t_, k]) for k, t_ in at]
    assert t["below"].tolist() == [int(scores["below"][t_, k]) for k, t_ in at] and t["n"].tolist() == [int(scores["n"][t_, k]) for k, t_ in at]
