"""pileup of whole reads: the ragged paths of extend added to the table (docs/codecs.md §4.22; slow5tools_amd/csrc/pileup_kernels.hip, the
layout and the walk over its segments in ragged_dev.h).

The oracle is pileup_long_ref of pileup_ref.py: the definition of §4.22 in int64 numpy for the ragged layout, read by read, with the invariants
asserted.  It is tied to §4.18's restatement (pileup_ref, in the same file) on every case of that file re-laid as ragged.  Every member of the
table is an integer sum, minimum or maximum, so the device is held to it byte for byte, whatever the segment length, the window, the sort,
the grid, the calls and the streams.  The headers' plain C++ (ragged_dev.h, pileup_dev.h) is also compiled for the CPU, once more under the
address and undefined-behaviour sanitizers, and held to the same oracle with the segments visited in a shuffled order, each resolved by
seg_item, the one resolver the kernels walk with; seg_item itself is held to a plain double loop over reads and segments.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from chain_common import BEHIND, DEFAULT_COLS, DEFAULT_GRID, DEFAULT_SEG, DEFAULT_SORT, DNA, EVENT, EXT_ROW, PATH_ROW, PATH_WIDE, PILE_COL, PILE_TOTAL, QUERY_SHORT, ROOT
from chain_common import Acc, host_build, levels_signal, pile_accum, pile_lines, record, synth_file
from chain_common import gpu  # noqa: F401
from dtw_ref import quant_ref
from pileup_ref import LongCase, _explain, _first_lo, flawed_long_cases, kernel_cases, layout_cases, long_cases, mixed_case, pileup_long_ref, pileup_ref, piling_case
from pileup_ref import relay, sums_long, table_bytes

_WANT = {}


def wanted(name, events=True):
    """the restatement of a case of long_cases(), computed once"""
    if (name, events) not in _WANT:
        _WANT[name, events] = table_bytes(pileup_long_ref(long_cases()[name], events))
    return _WANT[name, events]


# ---------------------------------------------------------------------------------------------------------------- not gpu

CALLS = ["s5gpu_pileup_long_work_bytes", "s5gpu_pileup_accum_long_dev", "s5gpu_pileup_open_whole", "s5gpu_pileup_add_batch_whole"]


def test_library_exports_the_whole_read_calls_and_the_tool_takes_whole(tmp_path):
    from slow5tools_amd import _lib, build, pileup

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in CALLS if s not in exported]
    assert not [s for s in CALLS if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert [len(getattr(L, s).argtypes) for s in CALLS] == [2, 16, 6, 9]
    for name in ("work_bytes_long", "accum_long_dev", "pileup_whole_dev", "PileupWhole"):
        assert hasattr(pileup, name), name
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "slow5gpu.h"\nint main(void){\n'
                   'size_t (*a)(uint32_t, uint64_t) = s5gpu_pileup_long_work_bytes;\n'
                   'int (*b)(uint32_t, const int16_t *, const uint64_t *, const uint32_t *, uint64_t, const int16_t *, uint32_t, const int32_t *, const int32_t *,'
                   ' const int32_t *, const s5gpu_event_t *, uint32_t, void *, size_t, void *, void *) = s5gpu_pileup_accum_long_dev;\n'
                   'void *(*c)(const s5gpu_event_params_t *, const s5gpu_map_params_t *, const s5gpu_band_params_t *, size_t, const int16_t *, uint32_t)'
                   ' = s5gpu_pileup_open_whole;\n'
                   'int (*d)(void *, uint32_t, const void *const *, const size_t *, int, int, s5gpu_map_row_t *, s5gpu_ext_row_t *, int32_t *)'
                   ' = s5gpu_pileup_add_batch_whole;\n'
                   'printf("%d\\n", a && b && c && d);return 0;}\n')
    here = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl"),
                           "-L", here, "-lslow5gpu", "-Wl,-rpath," + here])
    assert subprocess.check_output([str(tmp_path / "decl")], text=True).split() == ["1"]
    # the tool takes --whole: with a reference that does not exist it gets as far as opening it (exit 2, no usage line); its options without
    # --whole, and values outside their ranges, are usage errors
    p = subprocess.run([pileup.S5PILEUP, "--whole", "--tile", "64", "--band", "128", "--max-events", "5000", str(tmp_path / "none.txt"), str(tmp_path / "none.blow5")],
                       capture_output=True)
    assert p.returncode == 2 and b"usage" not in p.stderr and b"cannot open" in p.stderr, p.stderr
    for args in (["--tile", "64"], ["--whole", "--tile", "100"], ["--whole", "--band", "100"], ["--whole", "--max-events", "0"], ["--whole", "--band", "8192"],
                 ["--whole", "--max-events", str((1 << 20) + 1)]):
        p = subprocess.run([pileup.S5PILEUP] + args + [str(tmp_path / "none.txt"), str(tmp_path / "none.blow5")], capture_output=True)
        assert p.returncode == 2 and b"usage" in p.stderr and b"--whole" in p.stderr, (args, p.stderr)


def test_work_bytes():
    from slow5tools_amd import _lib, pileup

    f = _lib.lib().s5gpu_pileup_long_work_bytes
    assert f(0, 0) > 0 and f(1, 1 << 40) > 0 and f(1, (1 << 40) + 1) == 0
    # verdicts, the prefix, the sort's 2 x 1024 words and a (read, segment) for each of total_rows / 64 + n segments
    for n, total in ((1, 1), (5, 1000), (4096, 4096 * 16384), (1000, 0)):
        need = 4 * n + 8 * (n + 1) + 8 * 1024 + 8 * (total // 64 + n)
        assert need <= f(n, total) <= need + 64 and f(n, total) % 16 == 0 and pileup.work_bytes_long(n, total) == f(n, total), (n, total)


def test_refused_arguments_are_refused_before_a_device_is_needed():
    """S5GPU_ERR_ARG (-1) and S5GPU_ERR_NOMEM (-3) of the ragged call (the pointers are never dereferenced on the host, so made-up aligned
    addresses serve), and the refusals of open_whole and of the adds"""
    from slow5tools_amd import _lib

    L = _lib.lib()
    P = 1 << 20
    need = L.s5gpu_pileup_long_work_bytes(4, 1000)

    def accum(n=4, q=P, first=P, ql=P, total=1000, ref=P, R=100, lo=P, hi=P, st=P, ev=P, skip=0, work=P, wb=need, acc=P):
        return L.s5gpu_pileup_accum_long_dev(n, q, first, ql, total, ref, R, lo, hi, st, ev, skip, work, wb, acc, None)
    assert accum(R=0) == -1 and accum(R=(1 << 26) + 1) == -1 and accum(total=(1 << 40) + 1) == -1
    for name in ("q", "first", "ql", "ref", "lo", "hi", "st", "work", "acc"):
        assert accum(**{name: None}) == -1, name
    assert accum(q=P + 1) == -1 and accum(first=P + 4) == -1 and accum(ql=P + 2) == -1 and accum(ref=P + 1) == -1 and accum(lo=P + 2) == -1
    assert accum(hi=P + 1) == -1 and accum(st=P + 2) == -1 and accum(ev=P + 8) == -1 and accum(work=P + 8) == -1 and accum(acc=P + 8) == -1
    assert accum(wb=need - 1) == -3 and accum(wb=0) == -3
    assert accum(n=0) == 0 and accum(n=0, q=None, first=None, lo=None, work=None, wb=0) == 0      # nothing to do: nothing is launched
    assert accum(n=0, acc=None) == -1 and accum(n=0, R=0) == -1
    vp = C.c_void_p
    h_ref = np.zeros(100, dtype=np.int16)

    def opened(mp=(0, 64, 10, 32.0, 127, 1), bp=(0, 10, 1 << 20, 256, 512, 127, 32.0), ev=(3, 6, 1.4, 9.0, 0.2), R=100, ref=True, bp_null=False):
        e, m, b = _lib.EventParams(*ev), _lib.MapParams(*mp), _lib.BandParams(*bp)
        h = L.s5gpu_pileup_open_whole(C.byref(e), C.byref(m), None if bp_null else C.byref(b), 0, h_ref.ctypes.data_as(vp) if ref else None, R)
        return h, L.s5gpu_last_error()
    for kw in (dict(bp_null=True), dict(bp=(0, 10, 1 << 20, 100, 512, 127, 32.0)), dict(bp=(0, 10, 1 << 20, 256, 100, 127, 32.0)),
               dict(bp=(0, 10, (1 << 20) + 1, 256, 512, 127, 32.0)), dict(bp=(1, 10, 1 << 20, 256, 512, 127, 32.0)), dict(bp=(0, 10, 1 << 20, 256, 512, 100, 32.0)),
               dict(bp=(0, 10, 1 << 20, 256, 512, 127, 16.0)), dict(mp=(0, 0, 1, 32.0, 127, 1)), dict(R=0), dict(R=(1 << 26) + 1), dict(ref=False)):
        h, why = opened(**kw)
        assert h is None and why.startswith(b"s5gpu_pileup_open_whole:") and b"device" not in why, (kw, why)
    assert L.s5gpu_pileup_add_batch_whole(None, 0, None, None, 1, 1, None, None, None) == -1


def test_the_options_refuse_bad_values():
    from slow5tools_amd import _lib

    L = _lib.lib()
    for key, bad, good in ((b"pileup_long_seg", (-1, 0, 1, 32, 63, 65, 96, 1000, 2048), (64, 128, 256, 512, 1024, DEFAULT_SEG)),
                           (b"pileup_long_cols", (-1, 1, 32, 63, 65, 96, 1000, 2048), (0, 64, 128, 256, 512, 1024, DEFAULT_COLS)),
                           (b"pileup_long_sort", (-1, 2), (0, 1, DEFAULT_SORT)),
                           (b"pileup_long_grid", (0, -1, 1025), (1, 7, 1024, DEFAULT_GRID))):
        for v in bad:
            assert L.s5gpu_set_option(key, v) == -1, (key, v)
        for v in good:                                                     # (the defaults last)
            assert L.s5gpu_set_option(key, v) == 0, (key, v)
    for key, v in ((b"pileup_lds_cols", DEFAULT_COLS), (b"pileup_grid", DEFAULT_GRID)):     # the old keys keep their meaning
        assert L.s5gpu_set_option(key, v) == 0


def test_restatement_on_hand_made_paths_and_against_the_fixed_pitch_one():
    # the two reads of test_pileup's hand-made case, ragged, the first with its event rows 2 further on
    q = np.array([10, 20, 30, 0, 0, 5, -5], dtype=np.int16)
    lo, hi = np.array([0, 1, 2, BEHIND, BEHIND, 1, 2], dtype=np.int32), np.array([1, 1, 4, BEHIND, BEHIND, 1, 2], dtype=np.int32)
    ev = np.zeros(7, dtype=EVENT)
    ev["length"] = [4, 5, 6, 0, 0, 7, 8]
    total, cols = pileup_long_ref(LongCase(q, [0, 5, 7], [3, 2], [1, 2, 3, 4, 5, 6], lo, hi, ev=ev))
    assert cols["depth"].tolist() == [1, 2, 2, 1, 1, 0] and cols["n_events"].tolist() == [1, 3, 2, 1, 1, 0]
    assert cols["n_samples"].tolist() == [4, 4 + 5 + 7, 6 + 8, 6, 6, 0] and cols["sum_cost"].tolist() == [9, 8 + 18 + 3, 27 + 8, 26, 25, 0]
    assert tuple(total)[:6] == (2, 0, 0, 8, 124, 6)
    # every case of the fixed-pitch list, re-laid: the two definitions agree
    for name, case in kernel_cases().items():
        for events in (True, False):
            want = table_bytes(pileup_ref(case, events))
            for ev_skip in (0, 3):
                got = table_bytes(pileup_long_ref(relay(case, ev_skip), events))
                assert got == want, (name, events, ev_skip, _explain(got, want))
    # the case makers make what they promise
    for name, (c, skipped, bad) in flawed_long_cases().items():
        t, _ = pileup_long_ref(c)
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (3 - skipped - bad, skipped, bad), name
    valid = np.frombuffer(wanted("flawed: valid")[64:], PILE_COL)
    for name, (c, bad_read) in layout_cases().items():
        t, _ = pileup_long_ref(c)
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (c.n - 1, 0, 1), name
        d = c.copy()
        d.status[bad_read] = 5                                             # the same table but for the count: the neighbours are intact
        t2, cols2 = pileup_long_ref(d)
        assert table_bytes(pileup_long_ref(c))[64:] == cols2.tobytes() and t2["reads_skipped"] == 1, name
    assert valid["depth"].max() >= 1
    t, cols = pileup_long_ref(sums_long())
    assert cols["sumsq_q"][0] == 65536 * 32767 ** 2 > 2 ** 45 and cols["sum_cost"][0] == 65536 * 65535 and cols["depth"][0] == 1
    t, cols = pileup_long_ref(piling_case())
    assert np.flatnonzero(cols["n_events"]).min() >= 100 and np.flatnonzero(cols["n_events"]).max() <= 399 and cols["depth"].max() == 48
    assert np.frombuffer(wanted("empty batch")[:64], PILE_TOTAL)[0]["reads_used"] == 0


PILE_LONG_HOST = r'''
// The whole-read code of ragged_dev.h and pileup_dev.h on the CPU, with plain adds in place of the atomics: what k_pileup_long_plan, _check,
// the sort and _accum do with it, every table allocated at exactly its size, the segments visited in a shuffled order (or in the sort's),
// every one resolved by seg_item, the kernels' own resolver, which is also held to a plain double loop (brute).
// in.bin: n, R, events?, ev_skip, S, cols, wlo, sort, seed, pad (uint32), total_rows (uint64), then first, qlen, status, queries, ref, lo, hi,
// events; out.bin: the accumulator's bytes.
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
static T *get(FILE *f, size_t k) {                                          // exactly k elements
    T *p = (T *)malloc(k ? k * sizeof(T) : 1);
    if (!p || (k && fread(p, sizeof(T), k, f) != k)) abort();
    return p;
}
static uint64_t g_rand;
static uint64_t rnd() { g_rand = g_rand * 6364136223846793005ull + 1442695040888963407ull; return g_rand >> 33; }
static void shuffle(uint64_t *v, uint64_t k) { for (uint64_t i = k; i > 1; i--) { const uint64_t j = rnd() % i, t = v[i - 1]; v[i - 1] = v[j]; v[j] = t; } }

// seg_item against a plain double loop over the reads and their segments of S rows (verdict: the layout's): in P's order with "none yet"
// before each item (0) and with the read carried from the item before (1), and through an ordered list, the double loop's backwards (2)
static bool brute(const PileLongArgs &A, const uint32_t *verdict, uint32_t S) {
    std::vector<uint64_t> P(A.n + 1ull), want;
    for (uint32_t k = 0; k < A.n; k++) {
        P[k] = want.size();
        for (uint32_t s = 0; verdict[k] == V_USED && s < segs_of(A.qlen[k], S); s++) want.push_back((uint64_t)k << 32 | s);
    }
    P[A.n] = want.size();
    std::vector<uint64_t> order(want.rbegin(), want.rend());
    const LongPtrs L = {nullptr, P.data(), nullptr, nullptr, order.data(), order.size()};
    Seg carried = seg_none(A.n);
    for (uint64_t it = 0; it < want.size(); it++)
        for (int mode = 0; mode < 3; mode++) {
            Seg fresh = seg_none(A.n), *g = mode == 1 ? &carried : &fresh;
            const uint64_t w = mode == 2 ? order[it] : want[it];
            const uint32_t k = (uint32_t)(w >> 32), s = (uint32_t)w, r0 = s * S, r1 = A.qlen[k] - r0 < S ? A.qlen[k] : r0 + S;
            if (!seg_item(A, S, L, mode == 2, it, g) || g->k != k || g->s != s || g->r0 != r0 || g->r1 != r1) return false;
        }
    Seg g = seg_none(A.n);
    return !seg_item(A, S, L, true, order.size(), &g);                       // a place behind the list's end stands for nothing
}

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    uint32_t h[10];
    uint64_t total_rows;
    if (!f || !o || fread(h, 4, 10, f) != 10 || fread(&total_rows, 8, 1, f) != 1) return 1;
    const uint32_t n = h[0], R = h[1], ev_skip = h[2] ? h[3] : 0u, S = h[4], cols = h[5], sort = h[7];
    g_rand = h[8];
    uint64_t *first = get<uint64_t>(f, (size_t)n + 1);
    uint32_t *qlen = get<uint32_t>(f, n);
    int32_t *status = get<int32_t>(f, n);
    int16_t *q = get<int16_t>(f, total_rows), *ref = get<int16_t>(f, R);
    int32_t *lo = get<int32_t>(f, total_rows), *hi = get<int32_t>(f, total_rows);
    s5gpu_event_t *ev = h[2] ? get<s5gpu_event_t>(f, total_rows) : nullptr;
    // the plan: the work area's parts, each at exactly its size
    const LongWork lw = long_work(n, total_rows);
    if (lw.o_prefix < 4ull * n || lw.o_hist < lw.o_prefix + 8ull * (n + 1ull) || lw.o_order < lw.o_cursor + 4ull * LONG_KEYS ||
        lw.bytes < lw.o_order + 8 * long_order_cap(n, total_rows))
        return 3;
    const PileLongArgs A = {n, q, first, qlen, total_rows, ref, R, lo, hi, status, ev, ev_skip, nullptr, nullptr};
    const uint64_t cap = long_order_cap(n, total_rows);
    uint32_t hist[LONG_KEYS], cursor[LONG_KEYS], *verdict = (uint32_t *)malloc(n ? 4ull * n : 1);
    uint64_t *P = (uint64_t *)malloc(8ull * (n + 1ull)), *order = (uint64_t *)malloc(cap ? 8 * cap : 1);   // an ordered list of exactly cap entries
    const LongPtrs L = {verdict, P, hist, cursor, order, cap};
    memset(hist, 0, sizeof hist);
    P[0] = 0;
    for (uint32_t k = 0; k < n; k++) {
        verdict[k] = long_verdict(first[k], first[k + 1], qlen[k], status[k], total_rows, ev_skip);
        P[k + 1] = P[k] + (verdict[k] == V_USED ? segs_of(qlen[k], S) : 0u);
    }
    if (!brute(A, verdict, 64u) || !brute(A, verdict, 256u)) return 7;
    const uint64_t total = P[n];
    // the check, in a shuffled order; seg_find and seg_next agree
    uint64_t *list = (uint64_t *)malloc(total ? 8 * total : 1);
    for (uint64_t g = 0; g < total; g++) list[g] = g;
    shuffle(list, total);
    const bool sorted = sort && total <= cap;
    uint32_t walk = 0;
    for (uint64_t g = 0; g < total; g++) {
        walk = seg_next(P, n, walk, g);
        if (walk != seg_find(P, n, g)) return 4;
    }
    for (uint64_t x = 0; x < total; x++) {
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, false, list[x], &g) || g.k != seg_find(P, n, list[x]) || verdict[g.k] & V_SKIPPED) return 4;
        if (g.r0 >= g.r1 || g.r1 > qlen[g.k] || g.r1 - g.r0 > S || g.r0 != g.s * S) return 4;
        if (!seg_rows_ok(g.r0, g.r1, 0, 1, lo + first[g.k], hi + first[g.k], R)) verdict[g.k] |= V_BAD;
        if (sorted) hist[seg_key(lo[first[g.k] + g.r0], R)]++;
    }
    if (sorted) {                                                           // the sort
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
    // the cells: through the ordered list, or in P's order shuffled
    s5gpu_pile_col_t *table = empty_cols(R), *win = empty_cols(cols);
    Window W;
    W.lo = h[6]; W.cols = cols;
    s5gpu_pile_total_t T;
    memset(&T, 0, sizeof T);
    T.R = R;
    uint32_t last_key = 0;
    for (uint64_t x = 0; x < total; x++) {
        Seg g = seg_none(n);
        if (!seg_item(A, S, L, sorted, sorted ? x : list[x], &g)) return 4;
        const uint32_t k = g.k;
        if (sorted) {
            const uint32_t key = seg_key(lo[first[k] + g.r0], R);
            if (key < last_key) return 6;                                   // the list is in the keys' order
            last_key = key;
        }
        if (verdict[k] != V_USED) continue;
        seg_cells<HostOps>(g.r0, g.r1, 0, 1, lo + first[k], hi + first[k], q + first[k], ev ? ev + first[k] + ev_skip : nullptr, ref, R, W, win, table, &T.cells,
                           &T.cost);
    }
    for (uint32_t b = 0; b < cols; b++) {
        const uint32_t j = W.lo + b;
        if (j >= W.lo && j < R) col_merge<HostOps>(table + j, win + b);
        else if (win[b].n_events) return 2;                                // a cell went to a slot that stands for no column
    }
    for (uint32_t k = 0; k < n; k++) {
        if (verdict[k] & V_SKIPPED) T.reads_skipped++;
        else if (verdict[k] & V_BAD) T.reads_bad++;
        else T.reads_used++;
    }
    fwrite(&T, sizeof T, 1, o);
    fwrite(table, sizeof *table, R, o);
    free(table); free(win); free(order); free(list); free(P); free(verdict); free(first); free(qlen); free(status); free(q); free(ref); free(lo); free(hi);
    free(ev);
    fclose(f);
    return fclose(o) == 0 ? 0 : 1;
}
'''


def _build_host(tmp_path, extra=()):
    return host_build(tmp_path, "pile_long_host", PILE_LONG_HOST, ["-O1", "-g", "-std=c++17", "-Wall"], extra)


def _run_host(exe, tmp_path, case, events=True, S=64, cols=0, wlo=0, sort=0, seed=1):
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(struct.pack("<10IQ", case.n, case.R, int(events), case.ev_skip, S, cols, wlo, sort, seed, 0, case.total))
        for a in (case.first, case.qlen, case.status, case.q, case.ref, case.lo, case.hi) + ((case.ev,) if events else ()):
            fh.write(a.tobytes())
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return (tmp_path / "out.bin").read_bytes()


def run_long_header_on_the_cpu(tmp_path, extra=(), thorough=True):
    exe = _build_host(tmp_path, extra)
    for name, case in long_cases().items():
        for events in (True, False):
            want = wanted(name, events)
            got = _run_host(exe, tmp_path, case, events)
            assert got == want, (name, events, _explain(got, want))
        if not thorough and case.total > 100000:
            continue
        for S, cols, wlo, sort, seed in ((64, 64, _first_lo(case), 1, 2), (256, 64, max(case.R - 10, 0), 0, 3), (1024, 1024, 0, 1, 4)):
            got = _run_host(exe, tmp_path, case, True, S, cols, wlo, sort, seed)
            assert got == wanted(name), (name, S, cols, wlo, sort, _explain(got, wanted(name)))


def test_the_header_code_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """long_verdict, segs_of, seg_find / seg_next, seg_item (against a plain double loop at S 64 and 256, from both start conventions and
    through an ordered list), seg_rows_ok and seg_cells (row_ok and row_cells with hi_prev from the ragged array), seg_key and the window of
    ragged_dev.h and pileup_dev.h as g++ compiles them, over the case list, segments in a shuffled order and in the sort's"""
    run_long_header_on_the_cpu(tmp_path)


def test_the_header_code_runs_clean_under_the_sanitizers(tmp_path):
    """the same stand-alone program under -fsanitize=address,undefined: every table is allocated at exactly its size"""
    run_long_header_on_the_cpu(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"), thorough=False)


# ---------------------------------------------------------------------------------------------------------------- gpu

def _options(env, seg=64, cols=DEFAULT_COLS, sort=DEFAULT_SORT, grid=DEFAULT_GRID):
    for key, v in ((b"pileup_long_seg", seg), (b"pileup_long_cols", cols), (b"pileup_long_sort", sort), (b"pileup_long_grid", grid)):
        env.lib.check(env.L.s5gpu_set_option(key, v), key.decode())


def _accum_long(env, acc, case, events=True, stream=None, sync=True, short=0, want_rc=0):
    """THE way into s5gpu_pileup_accum_long_dev here: the inputs uploaded, a work area of exactly the size asked for between guards, the call
    made on `stream`, and afterwards the guards and every input checked.  short: the bytes the call is told are missing."""
    torch = env.torch
    host = [case.q, case.first.view(np.int64), case.qlen.view(np.int32), case.ref, case.lo, case.hi, case.status]
    host += [case.ev.view(np.int32).reshape(case.total, 4)] if events else []
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in host]
    need = env.L.s5gpu_pileup_long_work_bytes(case.n, case.total)
    assert need % 16 == 0 and need > 0
    work = torch.full((need + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if t.numel() else None for t in dev] + ([] if events else [None])
    rc = env.L.s5gpu_pileup_accum_long_dev(case.n, ptr[0], ptr[1], ptr[2], case.total, ptr[3], case.R, ptr[4], ptr[5], ptr[6], ptr[7], case.ev_skip,
                                           work.data_ptr() + 64, need - short, acc.ptr, C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == want_rc, (rc, env.L.s5gpu_last_error())

    def check():
        for t, a in zip(dev, host):
            assert np.array_equal(t.cpu().numpy(), a), "an input was written"
        w = work.cpu().numpy()
        assert (w[:64] == 0x5A).all() and (w[-64:] == 0x5A).all(), "a guard of the work area was written"
        if want_rc != 0:
            assert (w == 0x5A).all(), "the work area was written by a call that was refused"
        return acc.bytes()
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


def _table(env, case, events=True, **opt):
    _options(env, **opt)
    try:
        return _accum_long(env, Acc(env, case.R), case, events)
    finally:
        _options(env, seg=DEFAULT_SEG)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(long_cases()))
def test_the_case_list_is_exact(gpu, name):
    case = long_cases()[name]
    for events in (True, False):
        for sort in (0, 1):
            got, want = _table(gpu, case, events, sort=sort), wanted(name, events)
            assert got == want, (events, sort, _explain(got, want))
    if name in ("mixed R=5000", "64-bit sums", "layout: Q = 2^20 + 1"):      # ... and at the shipped segment length
        got = _table(gpu, case, True, seg=DEFAULT_SEG)
        assert got == wanted(name), _explain(got, wanted(name))
    t = np.frombuffer(wanted(name)[:64], PILE_TOTAL)[0]
    if name.startswith("flawed: "):
        skipped, bad = flawed_long_cases()[name[8:]][1:]
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (3 - skipped - bad, skipped, bad)
    if name.startswith("layout: "):
        assert (t["reads_used"], t["reads_skipped"], t["reads_bad"]) == (case.n - 1, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["seams", "piling"])
def test_the_options_do_not_change_the_table(gpu, name):
    case, want = long_cases()[name], wanted(name)
    for seg in (64, 256, 1024):
        for cols in (0, 64, DEFAULT_COLS):
            for sort in (0, 1):
                for grid in (1, DEFAULT_GRID):
                    got = _table(gpu, case, True, seg=seg, cols=cols, sort=sort, grid=grid)
                    assert got == want, (seg, cols, sort, grid, _explain(got, want))


@pytest.mark.gpu
def test_short_reads_give_the_table_of_the_fixed_pitch_kernel(gpu):
    case = mixed_case(129, 200)
    fixed = pile_accum(gpu, Acc(gpu, case.R), case)
    for ev_skip in (0, 3):
        for sort in (0, 1):
            got = _table(gpu, relay(case, ev_skip), True, sort=sort)
            assert got == fixed, (ev_skip, sort, _explain(got, fixed))


@pytest.mark.gpu
def test_ragged_and_fixed_pitch_calls_share_an_accumulator(gpu):
    torch = gpu.torch
    case = mixed_case(129, 200)
    want = table_bytes(pileup_ref(case))
    a, b, c = relay(case.part(0, 60)), relay(case.part(60, 130), 3), case.part(130, 200)
    acc = Acc(gpu, case.R)
    _options(gpu)
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        checks = [_accum_long(gpu, acc, a, stream=s1, sync=False), _accum_long(gpu, acc, b, stream=s2, sync=False), pile_accum(gpu, acc, c, sync=False)]
        torch.cuda.synchronize()
        got = [f() for f in checks][-1]
        assert got == want, _explain(got, want)
        # a work area one byte short: S5GPU_ERR_NOMEM, and neither the accumulator nor the work area is touched
        assert _accum_long(gpu, acc, a, short=1, want_rc=-3) == want
    finally:
        _options(gpu, seg=DEFAULT_SEG)


@pytest.fixture(scope="module")
def chain(gpu):
    """five synthetic reads of about 3000 events, one of them too short for a query: the records, the reference, and the restatement fed with
    what extend_dev(host=False) returns for the batch"""
    torch = gpu.torch
    rng = np.random.default_rng(4022)
    lengths = [36000, 30000, 100, 40000, 33000]
    recs = [record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
    levels = rng.normal(500.0, 110.0, 3500).astype(np.float32)
    ref = quant_ref(levels)
    kw = dict(skip=2, qmax=100, qmin=20, tile_rows=64, band=128)
    dec = gpu.press.decode_to_device(recs)
    ev, first = gpu.events.events_dev(dec, DNA, "raw")
    out, x = gpu.extend.extend_dev(dec, ref, host=False, **kw)
    rows = x.rows.cpu().numpy().view(EXT_ROW).reshape(-1)
    case = LongCase(x.queries.cpu().numpy(), x.first.cpu().numpy().astype(np.uint64), x.qlen.cpu().numpy(), ref, x.lo.cpu().numpy(), x.hi.cpu().numpy(),
                    rows["status"], ev.cpu().numpy().view(EVENT).reshape(-1), kw["skip"])
    env = type("Chain", (), {})()
    env.recs, env.levels, env.ref, env.kw, env.dec, env.rows, env.case, env.want = recs, levels, ref, kw, dec, rows, case, pileup_long_ref(case)
    return env


@pytest.mark.gpu
def test_whole_reads_after_the_real_chain(gpu, chain):
    pl = gpu.pileup
    total, cols = chain.want
    used = chain.rows["status"] == 0
    assert used.tolist() == [True, True, False, True, True] and chain.rows["qlen"][used].min() > 2000 and total["reads_used"] == 4
    acc, st, ext = pl.pileup_whole_dev(chain.dec, chain.ref, pl.new_acc(len(chain.ref)), **chain.kw)
    got = table_bytes(pl.to_host(acc))
    assert got == table_bytes(chain.want), _explain(got, table_bytes(chain.want))
    assert st.cpu().numpy().tolist() == chain.rows["status"].tolist() and ext.cpu().numpy().view(EXT_ROW).reshape(-1).tolist() == chain.rows.tolist()
    assert total["cost"] == chain.rows["cost"][used].astype(np.int64).sum() and total["reads_used"] + total["reads_skipped"] + total["reads_bad"] == len(chain.recs)
    assert total["cells"] >= chain.rows["qlen"][used].sum() and (cols["n_samples"] >= cols["n_events"]).all() and total["reads_bad"] == 0


@pytest.mark.gpu
def test_the_whole_read_handle(gpu, chain):
    pl = gpu.pileup
    want = table_bytes(chain.want)
    with pl.PileupWhole(chain.ref, **chain.kw) as h:
        rc, map_rows, rows, status = h.add(chain.recs)
        assert rc == 0 and rows.tolist() == chain.rows.tolist() and status.tolist() == chain.rows["status"].tolist() and map_rows["qlen"].max() == 100
        got = table_bytes(h.close())
    assert got == want, _explain(got, want)
    h = pl.PileupWhole(chain.ref, **chain.kw)                              # two batches
    h.add(chain.recs[:2])
    h.add(chain.recs[2:])
    got = table_bytes(h.close())
    assert got == want, _explain(got, want)
    # the wrong add for a handle's kind is S5GPU_ERR_ARG, and the handle still closes with what it held
    h = pl.PileupWhole(chain.ref, **chain.kw)
    h.add(chain.recs)
    assert gpu.L.s5gpu_pileup_add_batch(h._h, 0, None, None, 1, 1, None, None) == -1
    assert table_bytes(h.close()) == want
    f = pl.Pileup(chain.ref, skip=2, qmax=100, qmin=20)
    assert gpu.L.s5gpu_pileup_add_batch_whole(f._h, 0, None, None, 1, 1, None, None, None) == -1
    t, _ = f.close()
    assert t["reads_used"] == 0
    # a corrupt record: -5, its status the decoder's, and the rest is accumulated
    recs = list(chain.recs)
    bad = bytearray(recs[1])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[1] = bytes(bad)
    d = chain.case.copy()
    d.status[1] = 5
    want_bad = table_bytes(pileup_long_ref(d))
    h = pl.PileupWhole(chain.ref, **chain.kw)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        h.add(recs)
    h.abandon()
    h = pl.PileupWhole(chain.ref, **chain.kw)
    rc, _, rows, status = h.add(recs, raise_on_error=False)
    assert rc == -5 and status[1] not in (0, QUERY_SHORT, PATH_WIDE, PATH_ROW) and rows["qlen"][1] == 0 and rows[[0, 2, 3, 4]].tolist() == chain.rows[[0, 2, 3, 4]].tolist()
    got = table_bytes(h.close())
    assert got == want_bad, _explain(got, want_bad)


@pytest.mark.gpu
def test_the_tool_with_and_without_whole(gpu, chain, tmp_path):
    pl = gpu.pileup
    ref_txt = tmp_path / "ref.txt"
    ref_txt.write_text("".join("%.9g\n" % v for v in chain.levels))
    synth_file(tmp_path / "reads.blow5", chain.recs)
    kw = chain.kw
    args = ["--skip", str(kw["skip"]), "--events", str(kw["qmax"]), "--min-events", str(kw["qmin"])]
    files = [str(ref_txt), str(tmp_path / "reads.blow5")]
    total, cols = chain.want
    p = subprocess.run([pl.S5PILEUP, "-K", "3", "--whole", "--tile", str(kw["tile_rows"]), "--band", str(kw["band"])] + args + files, capture_output=True, timeout=120)
    assert p.returncode == 0 and b"short" in p.stderr and b"reads used 4, skipped 1, bad 0" in p.stderr, p.stderr
    assert p.stdout == b"".join(pile_lines(chain.ref, cols)) and len(p.stdout.splitlines()) == int((cols["depth"] >= 1).sum()) > 100
    t = pl.file_pileup(files[1], files[0], batch=3, whole=True, tile_rows=kw["tile_rows"], band=kw["band"], skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"])
    at = np.flatnonzero(cols["depth"] >= 1)
    assert t["ref_pos"].tolist() == at.tolist() and t["events"].tolist() == cols["n_events"][at].tolist() and t["samples"].tolist() == cols["n_samples"][at].tolist()
    # without --whole: the table of Pileup, the read heads
    h = pl.Pileup(chain.ref, skip=kw["skip"], qmax=kw["qmax"], qmin=kw["qmin"])
    h.add(chain.recs)
    _, head_cols = h.close()
    p = subprocess.run([pl.S5PILEUP, "-K", "3"] + args + files, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"".join(pile_lines(chain.ref, head_cols)) and b"reads used 4, skipped 1, bad 0" in p.stderr, p.stderr
    assert head_cols["n_events"].sum() < cols["n_events"].sum() // 10
