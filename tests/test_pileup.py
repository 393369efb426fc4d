"""pileup: per-reference-position statistics of aligned events, accumulated on the device (docs/codecs.md §4.18;
slow5tools_amd/csrc/pileup_kernels.hip).

The oracle is pileup_ref in this file: the definition of §4.18 in int64 numpy, read by read, with the invariants asserted.  Every member of
the table is an integer sum, minimum or maximum, so the device is held to it byte for byte, whatever the window, the grid, the batches and
the streams.  Paths for the kernel tests are random valid monotone paths, not DTW's: the kernel only sees lo and hi.  The header's
validation, row accumulation, window and flush (pileup_dev.h) are plain C++: they are also compiled for the CPU and held to the same oracle.
"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import Blow5, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DNA = (3, 6, 1.4, 9.0, 0.2)
MAP_ROW = np.dtype([("cost", "<u4"), ("qlen", "<u4"), ("start", "<i4"), ("end", "<i4")])
EVENT = np.dtype([("start", "<u4"), ("length", "<u4"), ("mean", "<f4"), ("stdv", "<f4")])
PILE_COL = np.dtype([("depth", "<u4"), ("n_events", "<u4"), ("n_samples", "<u8"), ("sum_q", "<i8"), ("sumsq_q", "<u8"), ("sum_cost", "<u8"),
                     ("min_q", "<i4"), ("max_q", "<i4")])
PILE_TOTAL = np.dtype([("reads_used", "<u8"), ("reads_skipped", "<u8"), ("reads_bad", "<u8"), ("cells", "<u8"), ("cost", "<u8"), ("R", "<u4"),
                       ("reserved", "<u4", (5,))])
NO_COST = 0xFFFFFFFF
EMPTY = (NO_COST, 0, -1, -1)
QUERY_SHORT, PATH_WIDE, PATH_ROW = 18, 19, 20
QLENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 1024]      # (test_align.py) lanes hold 0 to 16 rows, both sides of every 64
KNOWN_SEED = 20261019
DEFAULT_COLS, DEFAULT_GRID = 1024, 1024                                    # the library's defaults (docs/codecs.md §4.18, Measured)
BEHIND = 0x7FFFFFF0                                                        # what lo and hi hold behind Q in these tests: never to be read


# ---------------------------------------------------------------------------------------------------------------- the restatement

def quant_ref(m, scale=32.0, clip=127):
    """quant of §4.16 (copied from test_align.py): float64, sums strictly left to right"""
    m = np.asarray(m, dtype=np.float32)
    L = len(m)
    q = np.zeros(L, dtype=np.int16)
    if L == 0:
        return q
    with np.errstate(all="ignore"):
        d = m.astype(np.float64)
        mu = np.cumsum(d)[-1] / np.float64(L)
        e = d - mu
        sd = np.sqrt(np.cumsum(e * e)[-1] / np.float64(L))
        if not (sd > 0.0 and np.isfinite(sd)):
            return q
        return np.clip(np.rint((e / sd) * np.float64(scale)), -clip, clip).astype(np.int16)


def sdtw_ref(q, r):
    """(cost, start, end) of §4.16 (copied from test_align.py): D and S filled along anti-diagonals, the predecessor of least D with ties to the
    diagonal, then (i - 1, j), then (i, j - 1)"""
    q = np.asarray(q).astype(np.int64)
    one = q.ndim == 1
    if one:
        q = q[None, :]
    r = np.asarray(r).astype(np.int64)
    B, Q = q.shape
    R = len(r)
    assert Q >= 1 and R >= 1
    INF = np.int64(1) << 40
    D = np.full((B, Q + 1, R + 1), INF, dtype=np.int64)
    S = np.full((B, Q + 1, R + 1), -1, dtype=np.int64)
    D[:, 0, :] = 0
    for k in range(Q + R - 1):
        i = np.arange(max(0, k - R + 1), min(Q - 1, k) + 1)
        j = k - i
        dg, up, lf = D[:, i, j], D[:, i, j + 1], D[:, i + 1, j]
        take_dg = (dg <= up) & (dg <= lf)
        take_up = ~take_dg & (up <= lf)
        D[:, i + 1, j + 1] = np.abs(q[:, i] - r[j][None, :]) + np.where(take_dg, dg, np.where(take_up, up, lf))
        s = np.where(take_dg, S[:, i, j], np.where(take_up, S[:, i, j + 1], S[:, i + 1, j]))
        S[:, i + 1, j + 1] = np.where((i == 0)[None, :], j[None, :], s)
    last = D[:, Q, 1:]
    assert last.max() <= 65535 * Q < 2 ** 26
    end = np.argmin(last, axis=1)
    b = np.arange(B)
    cost, start = last[b, end], S[b, Q, end + 1]
    return (int(cost[0]), int(start[0]), int(end[0])) if one else (cost, start, end)


def path_ref(q, r):
    """(cost, lo, hi) of §4.17 for ONE query (copied from test_align.py): the full D in int64, filled along anti-diagonals; the walk from
    (Q - 1, end) takes the predecessor of least D, ties to the diagonal, then (i - 1, j), then (i, j - 1), until row 0"""
    q = np.asarray(q).astype(np.int64)
    r = np.asarray(r).astype(np.int64)
    Q, R = len(q), len(r)
    assert q.ndim == 1 and Q >= 1 and R >= 1
    INF = np.int64(1) << 40
    D = np.full((Q + 1, R + 1), INF, dtype=np.int64)                       # D[i + 1, j + 1] is D[i][j]; row 0: "a path starts here"
    D[0, :] = 0
    c = np.abs(q[:, None] - r[None, :])
    for k in range(Q + R - 1):
        i = np.arange(max(0, k - R + 1), min(Q - 1, k) + 1)
        j = k - i
        D[i + 1, j + 1] = c[i, j] + np.minimum(np.minimum(D[i, j], D[i, j + 1]), D[i + 1, j])
    end = int(np.argmin(D[Q, 1:]))
    cost = int(D[Q, end + 1])
    lo, hi = np.full(Q, -1, dtype=np.int64), np.full(Q, -1, dtype=np.int64)
    i, j, total = Q - 1, end, 0
    hi[i] = j
    while True:
        total += int(c[i, j])
        if i == 0:
            lo[0] = j
            break
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]
        if dg <= up and dg <= lf:
            lo[i] = j
            i, j = i - 1, j - 1
            hi[i] = j
        elif up <= lf:
            lo[i] = j
            i -= 1
            hi[i] = j
        else:
            j -= 1
    assert total == cost and hi[Q - 1] == end and (lo <= hi).all() and (lo >= 0).all()
    assert set((lo[1:] - hi[:-1]).tolist()) <= {0, 1}
    assert sum(int(c[i, lo[i]:hi[i] + 1].sum()) for i in range(Q)) == cost
    assert sdtw_ref(q, r) == (cost, int(lo[0]), end)
    return cost, lo.astype(np.int32), hi.astype(np.int32)


def known_answer_cases(n_draws=40):
    """§4.16's known answer (copied from test_align.py): a reference of 1200 levels, neighbours at least 20 apart; a query that is the slice
    [a, a + Q) with every level but the first and the last held 1 to 3 times aligns at cost 0 from a to a + Q - 1.
    -> (ref, [(query, a, Q, rep)])"""
    rng = np.random.default_rng(KNOWN_SEED)
    lv = [int(rng.integers(-100, 101))]
    while len(lv) < 1200:
        v = int(rng.integers(-100, 101))
        if abs(v - lv[-1]) >= 20:
            lv.append(v)
    ref = np.array(lv, dtype=np.int16)
    cases = []
    for _ in range(n_draws):
        Q = int(rng.integers(2, 131))
        a = int(rng.integers(0, 1200 - Q + 1))
        rep = rng.integers(1, 4, Q)
        rep[0] = rep[-1] = 1
        piece = ref[a:a + Q]
        occurrences = sum(np.array_equal(ref[k:k + Q], piece) for k in range(1200 - Q + 1))
        if occurrences == 1:
            cases.append((np.repeat(piece, rep).astype(np.int16), a, Q, rep))
    return ref, cases


def levels_signal(n, rng):
    """a raw signal of random levels of dwell 4 .. 20 with a little noise: an event every dozen samples (copied from test_align.py)"""
    lv = []
    while len(lv) < n:
        lv += [int(rng.integers(300, 700))] * int(rng.integers(4, 21))
    return np.round(np.array(lv[:n], dtype=np.float64) + rng.normal(0.0, 3.0, n)).astype(np.int16)


class Case:
    """the inputs of s5gpu_pileup_accum_dev on the host: qm [n, pitch] int16, qlen [n], ref [R] int16, lo, hi [n, pitch] int32, status [n]
    int32, ev [n, pitch] EVENT"""

    def __init__(self, qm, qlen, ref, lo, hi, status=None, ev=None):
        self.qm = np.ascontiguousarray(qm, dtype=np.int16)
        self.n, self.pitch = self.qm.shape
        self.qlen = np.asarray(qlen, dtype=np.uint32).copy()
        self.ref = np.ascontiguousarray(ref, dtype=np.int16)
        self.R = len(self.ref)
        self.lo, self.hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
        self.status = np.zeros(self.n, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32).copy()
        if ev is None:
            ev = np.zeros((self.n, self.pitch), dtype=EVENT)
            ev["length"] = np.random.default_rng(self.n * 31 + self.R).integers(1, 5000, (self.n, self.pitch))
            ev["start"], ev["mean"], ev["stdv"] = 7, 1.5, 0.25
        self.ev = np.ascontiguousarray(ev, dtype=EVENT)
        assert self.lo.shape == self.hi.shape == self.ev.shape == (self.n, self.pitch) and len(self.qlen) == len(self.status) == self.n

    def part(self, a, b):
        return Case(self.qm[a:b], self.qlen[a:b], self.ref, self.lo[a:b], self.hi[a:b], self.status[a:b], self.ev[a:b])

    def copy(self):
        return Case(self.qm.copy(), self.qlen, self.ref.copy(), self.lo.copy(), self.hi.copy(), self.status, self.ev.copy())


def pileup_ref(case, events=True):
    """(total, cols) of §4.18 for a Case: a PILE_TOTAL record and a PILE_COL array.  int64 numpy, a read at a time; the invariants asserted."""
    R = case.R
    r = case.ref.astype(np.int64)
    depth, n_events, n_samples = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    sum_q, sumsq_q, sum_cost = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    min_q, max_q = np.full(R, 32767, np.int64), np.full(R, -32768, np.int64)
    used = skipped = bad = cells = cost = spans = 0
    for k in range(case.n):
        Q = min(int(case.qlen[k]), case.pitch)
        assert Q <= 1024
        if case.status[k] != 0 or Q == 0:
            skipped += 1
            continue
        lo, hi = case.lo[k, :Q].astype(np.int64), case.hi[k, :Q].astype(np.int64)
        ok = ((0 <= lo) & (lo <= hi) & (hi < R)).all()
        ok = ok and bool(np.isin(lo[1:] - hi[:-1], (0, 1)).all())
        if not ok:
            bad += 1
            continue
        used += 1
        w = hi - lo + 1
        i = np.repeat(np.arange(Q), w)                                     # the cells (i, j), row by row
        j = lo[i] + np.arange(w.sum()) - np.repeat(np.cumsum(w) - w, w)
        assert (j >= lo[i]).all() and (j <= hi[i]).all() and len(j) <= Q + R
        first = (i == 0) | (j > hi[np.maximum(i - 1, 0)])
        q = case.qm[k, :Q].astype(np.int64)[i]
        c = np.abs(q - r[j])
        np.add.at(depth, j, first.astype(np.int64))
        np.add.at(n_events, j, 1)
        if events:
            np.add.at(n_samples, j, case.ev["length"][k, :Q].astype(np.int64)[i])
        np.add.at(sum_q, j, q)
        np.add.at(sumsq_q, j, q * q)
        np.add.at(sum_cost, j, c)
        np.minimum.at(min_q, j, q)
        np.maximum.at(max_q, j, q)
        cells += len(j)
        cost += int(c.sum())
        spans += int(hi[Q - 1] - lo[0] + 1)
        assert int(first.sum()) == int(hi[Q - 1] - lo[0] + 1)              # a read is first once in every column it covers
    assert int(n_events.sum()) == cells and int(sum_cost.sum()) == cost and int(depth.sum()) == spans
    assert used + skipped + bad == case.n and (depth <= n_events).all() and n_events.max(initial=0) < 2 ** 32 and sumsq_q.min(initial=0) >= 0
    cols = np.zeros(R, dtype=PILE_COL)
    for name, a in (("depth", depth), ("n_events", n_events), ("n_samples", n_samples), ("sum_q", sum_q), ("sumsq_q", sumsq_q), ("sum_cost", sum_cost),
                    ("min_q", min_q), ("max_q", max_q)):
        cols[name] = a
    total = np.zeros(1, dtype=PILE_TOTAL)
    total[0] = (used, skipped, bad, cells, cost, R, (0, 0, 0, 0, 0))
    return total[0], cols


def table_bytes(want):
    total, cols = want
    return np.array([total], dtype=PILE_TOTAL).tobytes() + cols.tobytes()


def _explain(got, want):
    """where two tables differ, for an assertion's message"""
    if len(got) != len(want):
        return "sizes %d, %d" % (len(got), len(want))
    gt, wt = np.frombuffer(got[:64], PILE_TOTAL)[0], np.frombuffer(want[:64], PILE_TOTAL)[0]
    if gt.tobytes() != wt.tobytes():
        return "totals %s, want %s" % (gt, wt)
    gc, wc = np.frombuffer(got[64:], PILE_COL), np.frombuffer(want[64:], PILE_COL)
    j = int(np.flatnonzero(gc != wc)[0]) if (gc != wc).any() else -1
    return "column %d: %s, want %s" % (j, gc[j], wc[j])


def random_paths(rng, qlens, R, pitch, start=None, cap=None):
    """lo, hi [n, pitch] of random valid monotone paths: lo[0] random (or start[k]), per row a step of 0 or 1 and a span of 1 to 4, columns
    capped at cap (R - 1); BEHIND behind Q"""
    n = len(qlens)
    cap = R - 1 if cap is None else cap
    lo, hi = np.full((n, pitch), BEHIND, dtype=np.int32), np.full((n, pitch), BEHIND, dtype=np.int32)
    for k, ql in enumerate(qlens):
        Q = min(int(ql), pitch)
        if Q == 0:
            continue
        step, span = rng.integers(0, 2, Q), rng.integers(1, 5, Q)
        at = int(rng.integers(0, cap + 1)) if start is None else int(start[k])
        for i in range(Q):
            l = at if i == 0 else min(at + int(step[i]), cap)
            at = min(l + int(span[i]) - 1, cap)
            lo[k, i], hi[k, i] = l, at
    return lo, hi


def random_case(seed, qlens, R, pitch=None, start=None, cap=None, lohi=127):
    rng = np.random.default_rng(seed)
    pitch = max(max(qlens), 1) if pitch is None else pitch
    n = len(qlens)
    qm = rng.integers(-lohi, lohi + 1, (n, pitch)).astype(np.int16)
    ref = rng.integers(-lohi, lohi + 1, R).astype(np.int16)
    lo, hi = random_paths(rng, qlens, R, pitch, start, cap)
    return Case(qm, qlens, ref, lo, hi)


def mixed_case(R, n):
    """n = 16: one read of every length of QLENS; n = 200: lengths drawn from QLENS"""
    qlens = list(QLENS) if n == len(QLENS) else np.random.default_rng(n).choice(QLENS, n).tolist()
    return random_case(1000 + R + n, qlens, R, pitch=1024)


def pitch40_case():
    """a pitch of 40 with a qlen above it: Q is the pitch"""
    qlens = [40] * 30 + [64, 1000, 0, 7]
    return random_case(40, qlens, 129, pitch=40)


def window_case():
    """at a window of 64 columns and one workgroup the window is [200, 264): the first four reads anchor it; then reads that straddle its
    low and its high edge, reads wholly outside on either side, and one row that spans 300 columns across both edges"""
    R, Q = 500, 20
    starts = [200, 205, 230, 201] + [190, 185, 195] + [250, 255, 260] + [10, 300, 400, 120] + [150]
    c = random_case(77, [Q] * len(starts), R, start=starts)
    k = len(starts) - 1                                                     # the wide row: rows 0 .. 4 at 150, row 5 over 150 .. 449, the rest at 449
    c.lo[k, :Q], c.hi[k, :Q] = 150, 150
    c.hi[k, 5] = 449
    c.lo[k, 6:Q], c.hi[k, 6:Q] = 449, 449
    lo, hi = c.lo[:, :Q], c.hi[:, :Q]
    assert lo[:4, 0].min() == 200 and (lo[4:7, 0] < 200).all() and (hi[4:7, Q - 1] >= 200).all() and (hi[7:10, Q - 1] >= 264).all()
    assert hi[10, Q - 1] < 200 and (lo[11:13, 0] >= 264).all() and hi[13, Q - 1] < 200 and hi[k, 5] - lo[k, 5] + 1 == 300
    return c


def same_columns_case():
    """target enrichment: every read on the same 30 columns"""
    rng = np.random.default_rng(30)
    n, Q = 48, 70
    return random_case(31, [Q] * n, 400, start=rng.integers(100, 104, n), cap=129)


def sums_case():
    """64 reads of 1024 rows, every q = 32767, on a reference of one level -32768: sumsq_q of column 0 is above 2^45"""
    n, Q = 64, 1024
    return Case(np.full((n, Q), 32767, np.int16), [Q] * n, [-32768], np.zeros((n, Q), np.int32), np.zeros((n, Q), np.int32))


def flawed_cases():
    """{name: (Case, skipped, bad)}: a batch of 12 valid reads of 130 rows (row 64 is lane 0's second) with read 5 made skipped or bad"""
    R, Q, at = 300, 130, 5
    base = random_case(12, [Q] * 12, R, cap=R - 10)
    assert base.hi[at, 40] >= 1
    out = {}

    def put(name, skipped, bad, f):
        c = base.copy()
        f(c)
        out[name] = (c, skipped, bad)
    put("valid", 0, 0, lambda c: None)
    for s in (QUERY_SHORT, PATH_WIDE, PATH_ROW, 5):
        put("status %d" % s, 1, 0, lambda c, s=s: c.status.__setitem__(at, s))
    put("qlen 0", 1, 0, lambda c: c.qlen.__setitem__(at, 0))
    put("lo -1", 0, 1, lambda c: c.lo.__setitem__((at, 3), -1))
    put("hi R", 0, 1, lambda c: c.hi.__setitem__((at, Q - 1), R))
    put("hi far", 0, 1, lambda c: c.hi.__setitem__((at, Q - 1), 0x7FFFFFFF))
    put("lo > hi", 0, 1, lambda c: c.lo.__setitem__((at, 9), c.hi[at, 9] + 1))

    def gap2(c):                                                            # rows 40 .. move right by 2: only the gap rule fails, at row 40
        c.lo[at, 40:Q] += 2
        c.hi[at, 40:Q] += 2
    put("gap 2", 0, 1, gap2)
    put("step back", 0, 1, lambda c: c.lo.__setitem__((at, 40), c.hi[at, 39] - 1))
    put("row 64 only", 0, 1, lambda c: c.lo.__setitem__((at, 64), -1))
    return out


def kernel_cases():
    """the cases of the GPU list that are small enough to run everywhere: {name: Case}"""
    cases = {"mixed R=%d" % R: mixed_case(R, 16) for R in (1, 65, 129, 5000)}
    cases.update({"pitch 40": pitch40_case(), "window edges": window_case(), "same 30 columns": same_columns_case(), "64-bit sums": sums_case()})
    cases.update({"flawed: " + k: v[0] for k, v in flawed_cases().items()})
    return cases


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
    (tmp_path / "pile_host.cpp").write_text(PILE_HOST)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *extra, "-I", os.path.join(ROOT, "slow5tools_amd", "csrc"), str(tmp_path / "pile_host.cpp"),
                           "-o", str(tmp_path / "pile_host")])
    return str(tmp_path / "pile_host")


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

@pytest.fixture(scope="module")
def gpu():
    import torch
    from slow5tools_amd import _lib, align, events, pileup, press
    from slow5tools_amd import map as smap

    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.press, env.events, env.map, env.align, env.pileup = torch, _lib, _lib.lib(), press, events, smap, align, pileup
    return env


def _options(env, cols=DEFAULT_COLS, grid=DEFAULT_GRID):
    env.lib.check(env.L.s5gpu_set_option(b"pileup_lds_cols", cols), "pileup_lds_cols")
    env.lib.check(env.L.s5gpu_set_option(b"pileup_grid", grid), "pileup_grid")


class Acc:
    """an accumulator of R columns on the device between two guards of 64 bytes of 0x5A, reset"""

    def __init__(self, env, R):
        self.env, self.R, self.nb = env, R, 64 + 48 * R
        self.t = env.torch.full((self.nb + 128,), 0x5A, dtype=env.torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr() + 64
        assert self.ptr % 16 == 0 and env.L.s5gpu_pileup_bytes(R) == self.nb
        self.reset()

    def reset(self):
        self.env.lib.check(self.env.L.s5gpu_pileup_reset_dev(self.ptr, self.R, None), "s5gpu_pileup_reset_dev")

    def bytes(self):
        self.env.torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        assert (h[:64] == 0x5A).all() and (h[-64:] == 0x5A).all(), "a guard of the accumulator was written"
        return h[64:-64].tobytes()


def _accum(env, acc, case, events=True, stream=None, sync=True):
    """THE way into s5gpu_pileup_accum_dev here: the inputs uploaded, the call made on `stream`, and afterwards the guards around acc and
    every input tensor checked.  sync=False: the caller synchronises and calls the returned check itself (the two-stream test)."""
    torch = env.torch
    host = [case.qm, case.qlen.view(np.int32), case.ref, case.lo, case.hi, case.status] + ([case.ev.view(np.int32).reshape(case.n, case.pitch, 4)] if events else [])
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in host]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev] + ([] if events else [None])
    rc = env.L.s5gpu_pileup_accum_dev(case.n, ptr[0], case.pitch, ptr[1], ptr[2], case.R, ptr[3], ptr[4], ptr[5], ptr[6], acc.ptr,
                                      C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert rc == 0, env.L.s5gpu_last_error()

    def check():
        for t, a in zip(dev, host):
            assert np.array_equal(t.cpu().numpy(), a), "an input was written"
        return acc.bytes()
    if not sync:
        return check
    torch.cuda.synchronize()
    return check()


def _table(env, case, events=True, cols=DEFAULT_COLS, grid=DEFAULT_GRID):
    _options(env, cols, grid)
    try:
        return _accum(env, Acc(env, case.R), case, events)
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
    _accum(gpu, acc, a)
    got = _accum(gpu, acc, b)
    assert got == want, _explain(got, want)
    # the halves on two streams at once
    acc.reset()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    checks = [_accum(gpu, acc, a, stream=s1, sync=False), _accum(gpu, acc, b, stream=s2, sync=False)]
    torch.cuda.synchronize()
    got = [c() for c in checks][-1]
    assert got == want, _explain(got, want)
    acc.reset()
    assert acc.bytes() == empty


@pytest.mark.gpu
def test_pileup_after_the_real_chain(gpu):
    """the warped slices of test_map.py through sdtw_dev, path_dev and accum_dev: every cost 0, depth the slices over a column, n_events the
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


def _record(i, sig):
    r, keep = ob.make_rec(ob.synth_read_id(i), 0, 8192.0, 23.0, 1467.61, 4000.0, sig)
    return ob.rec_to_mem(r, ob.REC_ZLIB, ob.SIG_SVB_ZD)[8:]


def _synth_file(path, recs):
    """a BLOW5 file of records without aux fields (copied from test_align.py): the header of a golden zlib + svb-zd file with the aux columns
    taken off its two '#' lines"""
    g = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    assert (g.rec_method, g.sig_method) == (1, 1)
    lines = g.header_text.split(b"\n")
    lines = [b"\t".join(l.split(b"\t")[:8]) if l.startswith(b"#") and b"\t" in l else l for l in lines]
    ht = b"\n".join(lines)
    body = b"".join(struct.pack("<Q", len(r)) + r for r in recs)
    with open(path, "wb") as fh:
        fh.write(g.raw[:64] + struct.pack("<I", len(ht)) + ht + body + b"5WOLB")


def _lines(ref, cols, min_depth=1):
    """the tool's lines, formatted from a table"""
    out = []
    for j in np.flatnonzero(cols["depth"] >= min_depth):
        c = cols[j]
        ne = float(c["n_events"])
        mean = float(c["sum_q"]) / ne
        var = float(c["sumsq_q"]) / ne - mean * mean
        out.append(b"%d\t%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%s\n" % (j, ref[j], c["depth"], c["n_events"], c["n_samples"], b"%.6g" % mean,
                                                                b"%.6g" % math.sqrt(max(var, 0.0)), c["min_q"], c["max_q"], b"%.6g" % (float(c["sum_cost"]) / ne)))
    return out


@pytest.mark.gpu
def test_pileup_end_to_end_on_a_synthetic_file(gpu, tmp_path):
    """Pileup.add in two batches, pileup_dev and s5pileup on the six reads of test_align.py, one record corrupt and one read too short: the
    same table, equal to pileup_ref on what align_dev returns"""
    torch, al, pl = gpu.torch, gpu.align, gpu.pileup
    rng = np.random.default_rng(41)
    lengths = [3000, 500, 40, 5000, 1500, 2500]
    recs = [_record(i, levels_signal(n, rng)) for i, n in enumerate(lengths)]
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
    _synth_file(tmp_path / "reads.blow5", recs)
    args = ["--skip", str(skip), "--events", str(qmax), "--min-events", str(qmin), str(ref_txt), str(tmp_path / "reads.blow5")]
    p = subprocess.run([pl.S5PILEUP, "-K", "4"] + args, capture_output=True, timeout=120)
    assert p.returncode == 1 and ids[3] in p.stderr and b"short" in p.stderr and b"reads used 4, skipped 2, bad 0" in p.stderr, p.stderr
    assert p.stdout == b"".join(_lines(ref, cols)) and len(p.stdout.splitlines()) == int((cols["depth"] >= 1).sum()) > 50
    p = subprocess.run([pl.S5PILEUP, "--min-depth", "2"] + args, capture_output=True, timeout=120)
    deep = _lines(ref, cols, 2)
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
