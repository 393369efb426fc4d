"""The restatements of sites (docs/codecs.md §4.25) in int64 numpy and Python integers, and the site lists the CPU and the GPU tests share:
cells_ref (the read x site matrix of a pileup_ref.LongCase), score_ref (its rows against a control's counts), and the planted case."""
import functools

import numpy as np

import contrast_ref as cr
from contrast_ref import BINS, hist_cases
from pileup_ref import LONG_QMAX, pileup_long_ref

SITE_CELL = np.dtype([("sum_q", "<i8"), ("cells", "<u4"), ("row0", "<u4")])
SITE_SCORE = np.dtype([("level", "<i2"), ("flags", "<u2"), ("below", "<u4"), ("above", "<u4"), ("n", "<u4")])
ROW_NONE, SAT = 0xFFFFFFFF, 2 ** 32 - 1
NO_CELL, EMPTY, COLUMN, HEAD = 1, 2, 64, 128


def verdicts_ref(case):
    """0 used, 1 skipped, 2 bad per read: the rule of §4.22 with ev_skip = 0, as hist_ref states it"""
    R, out = case.R, np.zeros(case.n, np.uint32)
    for k in range(case.n):
        Q, f0, f1 = int(case.qlen[k]), int(case.first[k]), int(case.first[k + 1])
        if case.status[k] != 0 or Q == 0:
            out[k] = 1
            continue
        if Q > LONG_QMAX or f0 > f1 or f1 > case.total or Q > f1 - f0:
            out[k] = 2
            continue
        lo, hi = case.lo[f0:f0 + Q].astype(np.int64), case.hi[f0:f0 + Q].astype(np.int64)
        if not (((0 <= lo) & (lo <= hi) & (hi < R)).all() and bool(np.isin(lo[1:] - hi[:-1], (0, 1)).all())):
            out[k] = 2
    return out


@functools.lru_cache(maxsize=None)
def _sums_of(name):
    """per column of a case of hist_cases(): (the cells of its histogram, the table's sum_q), for the invariants"""
    case, q0, shift = hist_cases()[name]
    counts = np.frombuffer(cr.wanted(name), "<u4")[16:].reshape(case.R, BINS).astype(np.int64).sum(axis=1)
    return counts, pileup_long_ref(case, events=False)[1]["sum_q"].astype(np.int64)


def cells_ref(case, sites, name=None):
    """the [M, n] SITE_CELL matrix of §4.25 for a LongCase and a strictly increasing list of columns below R.  name: the case's name in
    hist_cases(); the invariants against hist_ref and pileup_long_ref of the same case are then asserted for every site"""
    s = np.asarray(sites, dtype=np.int64)
    assert len(s) >= 1 and (s >= 0).all() and (s < case.R).all() and (np.diff(s) > 0).all()
    M = len(s)
    out = np.zeros((M, case.n), dtype=SITE_CELL)
    out["row0"] = ROW_NONE
    v = verdicts_ref(case)
    for k in np.flatnonzero(v == 0):
        Q, f0 = int(case.qlen[k]), int(case.first[k])
        lo, hi, q = case.lo[f0:f0 + Q].astype(np.int64), case.hi[f0:f0 + Q].astype(np.int64), case.q[f0:f0 + Q].astype(np.int64)
        near = np.flatnonzero((s >= lo[0]) & (s <= hi[-1]))                # (a site outside the read's span is crossed by no row)
        for t0 in range(0, len(near), 64):
            at = near[t0:t0 + 64]
            crosses = (lo[None, :] <= s[at, None]) & (s[at, None] <= hi[None, :])      # [sites, rows]
            cells = crosses.sum(axis=1)
            out["cells"][at, k] = cells
            out["sum_q"][at, k] = (crosses * q[None, :]).sum(axis=1)
            out["row0"][at, k] = np.where(cells > 0, crosses.argmax(axis=1), ROW_NONE)
        assert (out["cells"][near, k] > 0).all()                            # a valid path leaves no column of its span out
    if name is not None:
        counts, sum_q = _sums_of(name)
        assert out["cells"].astype(np.int64).sum(axis=1).tolist() == counts[s].tolist(), name
        assert out["sum_q"].sum(axis=1).tolist() == sum_q[s].tolist(), name
    assert ((out["cells"] == 0) == (out["row0"] == ROW_NONE)).all() and (out["sum_q"][out["cells"] == 0] == 0).all()
    return out


def level_ref(sum_q, cells):
    """floor((2 sum_q + cells) / (2 cells)) in Python integers (// is the floor, for negatives too): the mean rounded half up"""
    return (2 * int(sum_q) + int(cells)) // (2 * int(cells))


def score_ref(cells, sites, counts, q0, shift, R=None, bins=BINS):
    """the [M, n] SITE_SCORE rows of a SITE_CELL matrix against the control's counts [R', 64].  R: what the call is told, bins: what the head
    says, when they differ from R' and 64: the head then disagrees"""
    cells = np.asarray(cells)
    M, n = cells.shape
    R = len(counts) if R is None else R
    out = np.zeros((M, n), dtype=SITE_SCORE)
    if R != len(counts) or bins != BINS:
        out["flags"] = HEAD
        return out
    for t in range(M):
        col = int(sites[t]) < R
        C = [int(x) for x in counts[int(sites[t])]] if col else [0] * BINS
        total = sum(C)
        for k in range(n):
            c = cells[t, k]
            flags = (0 if col else COLUMN) | (EMPTY if total == 0 else 0)
            if c["cells"] == 0:
                out[t, k] = (0, flags | NO_CELL, 0, 0, min(total, SAT))
                continue
            level = level_ref(c["sum_q"], c["cells"])
            assert -32768 <= level <= 32767
            b = int(cr.bin_of(level, q0, shift))
            below, above = sum(C[:b + 1]), sum(C[b:])
            assert below + above == total + C[b]
            out[t, k] = (level, flags, min(below, SAT), min(above, SAT), min(total, SAT))
    return out


# ---------------------------------------------------------------------------------------------------------------- the site lists

def _span(case):
    """(the smallest lo, the largest hi) over the used reads of a case, or None"""
    v = verdicts_ref(case)
    ends = [(int(case.lo[int(case.first[k])]), int(case.hi[int(case.first[k]) + int(case.qlen[k]) - 1])) for k in np.flatnonzero(v == 0)]
    return (min(a for a, _ in ends), max(b for _, b in ends)) if ends else None


@functools.lru_cache(maxsize=None)
def site_lists(name):
    """{label: sites} for a case of hist_cases(): one site at column 0 and one at R - 1; up to 16 columns spread over the table; the columns
    left of every path and those right of every path (up to 16 each), where there are any; every column (M = R) for R of 1, 65 and 300; and by
    name the columns the issue asks for"""
    case, _, _ = hist_cases()[name]
    R = case.R
    out = {"column 0": [0], "column R - 1": [R - 1], "spread": sorted(set(int(x) for x in np.linspace(0, R - 1, 16)))}
    sp = _span(case)
    if sp and sp[0] > 0:
        out["left of every path"] = sorted(set(int(x) for x in np.linspace(0, sp[0] - 1, 16)))
    if sp and sp[1] < R - 1:
        out["right of every path"] = sorted(set(int(x) for x in np.linspace(sp[1] + 1, R - 1, 16)))
    if R in (1, 65, 300):
        out["every column"] = list(range(R))
    if name.startswith("edges R=300"):
        f = int(case.first[1])
        wide = int(np.argmax(case.hi[f:f + 65].astype(np.int64) - case.lo[f:f + 65]))
        assert case.hi[f + wide] - case.lo[f + wide] + 1 == 70
        out["inside the 70-wide row"] = [int(case.lo[f + wide]) + 35]
        out["the 64 piled reads"] = [40, 41, 42]
        assert all(int(case.lo[int(case.first[k])]) == 40 and int(case.hi[int(case.first[k]) + 2]) == 42 for k in range(3, 67))
    if name == "seams":
        f = int(case.first[1])                                              # the read that stays at rows 64 and 128
        assert case.lo[f + 64] == case.hi[f + 63] and case.lo[f + 128] == case.hi[f + 127]
        out["a stay across a seam"] = sorted({int(case.hi[f + 63]), int(case.hi[f + 127])})
        f0 = int(case.first[0])
        out["the 300-wide rows"] = [int(case.lo[f0 + 63]) + 150, int(case.lo[f0 + 64]) + 150]
        crossed = np.zeros(R, bool)
        for k in range(case.n):
            crossed[int(case.lo[int(case.first[k])]):int(case.hi[int(case.first[k]) + int(case.qlen[k]) - 1]) + 1] = True
        out["a column no read crosses"] = [int(np.flatnonzero(~crossed)[0]), int(np.flatnonzero(~crossed)[-1])]
    return out


_WANT = {}


def wanted(name, label):
    """the restatement's matrix of a case and one of its site lists, computed once (the invariants asserted)"""
    if (name, label) not in _WANT:
        _WANT[name, label] = cells_ref(hist_cases()[name][0], site_lists(name)[label], name)
    return _WANT[name, label]


# ---------------------------------------------------------------------------------------------------------------- hand-made controls

def score_hand_cases():
    """[(label, cells [M, n], sites, counts [R, 64], q0, shift, R told, the head's bins)]: control columns that are empty, all in one bin, entries whose
    bin is 0 and 63, a level at every edge of edge_levels, negative sums whose rounding is the floor, counts that saturate, a site at or
    beyond R, a head that disagrees, and 1000 random entries"""
    rng = np.random.default_rng(2525)
    out = []

    def entries(levels_and_cells):
        c = np.zeros(len(levels_and_cells), dtype=SITE_CELL)
        for i, (sum_q, cells) in enumerate(levels_and_cells):
            c[i] = (sum_q, cells, 5 if cells else ROW_NONE)
        return c
    for q0, shift in cr.BIN_PARAMS:
        e = [int(x) for x in cr.edge_levels(q0, shift)]
        row = entries([(v, 1) for v in e] + [(3 * v + 1, 3) for v in e if v < 32767] + [(3 * v - 1, 3) for v in e if v > -32768] + [(0, 0)] +
                      [(-1, 2), (-3, 2), (1, 2), (3, 2), (-7, 3), (-8, 3), (-2 * 32768, 2), (2 * 32767, 2), (-65535, 2), (65533, 2)])
        counts = rng.integers(0, 1000, (6, BINS)).astype(np.int64)
        counts[1] = 0                                                       # empty
        counts[2] = 0
        counts[2, 17] = 12345                                               # all in one bin
        counts[3] = 0
        counts[3, [0, 63]] = [7, 9]
        counts[4] = 2 ** 32 - 1                                             # every sum saturates
        counts[5] = 0
        counts[5, [3, 40]] = [2 ** 32 - 1, 1]                               # n saturates, a tail does not
        sites = list(range(6))
        out.append(("edges q0=%d shift=%d" % (q0, shift), np.stack([row] * 6), sites, counts, q0, shift, 6, BINS))
    row = entries([(-5, 2), (100, 1), (0, 0)])
    counts = rng.integers(0, 50, (3, BINS)).astype(np.int64)
    out.append(("a site at R", np.stack([row] * 2), [1, 3], counts, cr.Q0, cr.SHIFT, 3, BINS))   # column 3 is not read
    out.append(("a head of another R", np.stack([row] * 2), [1, 2], counts, cr.Q0, cr.SHIFT, 5, BINS))
    out.append(("a head of 32 bins", np.stack([row] * 2), [1, 2], counts, cr.Q0, cr.SHIFT, 3, 32))
    M, n = 10, 100                                                          # 1000 random entries: sparse and dense columns, small and large counts
    cells = np.zeros((M, n), dtype=SITE_CELL)
    k = rng.integers(0, 6, (M, n))
    k[rng.random((M, n)) < 0.1] = 0
    cells["cells"] = k
    cells["sum_q"] = rng.integers(-32768 * k.astype(np.int64), 32767 * k.astype(np.int64) + 1)
    cells["row0"] = np.where(k > 0, rng.integers(0, 1000, (M, n)), ROW_NONE)
    counts = rng.integers(0, 2 ** rng.integers(1, 31, (40, 1)), (40, BINS)) * (rng.random((40, BINS)) < rng.random((40, 1)))
    out.append(("1000 random entries", cells, sorted(rng.choice(40, M, replace=False).tolist()), counts.astype(np.int64), -300, 3, 40, BINS))
    return out


# ---------------------------------------------------------------------------------------------------------------- the planted case

PLANTED_SITES = list(range(cr.PLANTED_COLS[0], cr.PLANTED_COLS[1] + 1))


def planted_scores(paths=None):
    """-> (scores [10, 16], labels): the control is the histogram of reads 0 .. 7 of side 0; scored are reads 8 .. 11 of side 0 and all twelve
    of side 1 (labels 0 and 1) at columns 700 .. 709.  paths: [side][read] (lo, hi), the restatement's own by default"""
    ref, sides = cr.planted()
    paths = cr.planted_paths() if paths is None else paths
    _, control = cr.hist_ref(cr.planted_case(ref, sides[0][:8], paths[0][:8]))
    held = cr.planted_case(ref, sides[0][8:] + sides[1], list(paths[0][8:]) + list(paths[1]))
    cells = cells_ref(held, PLANTED_SITES)
    return score_ref(cells, PLANTED_SITES, control, cr.Q0, cr.SHIFT), cells, [0] * 4 + [1] * 12


def planted_condition(scores, cells, labels):
    """no read is left out, every read is covered at all ten sites, and every side-1 read has strictly more zero-tail sites than every
    held-out side-0 read; -> the zero-tail counts per read"""
    assert scores.shape == (10, 16) and (cells["cells"] > 0).all() and not (scores["flags"] != 0).any()
    zero = (np.minimum(scores["below"], scores["above"]) == 0).sum(axis=0)
    own, other = [int(z) for z, s in zip(zero, labels) if s == 0], [int(z) for z, s in zip(zero, labels) if s == 1]
    assert len(own) == 4 and len(other) == 12 and min(other) > max(own), (own, other)
    return own, other
