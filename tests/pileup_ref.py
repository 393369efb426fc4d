"""The restatements of pileup (docs/codecs.md §4.18) and of pileup over whole reads (§4.22) in int64 numpy, read by read, with the invariants
asserted, and the cases the CPU and the GPU tests share: Case and pileup_ref for the padded layout, LongCase and pileup_long_ref for the
ragged one, and relay, which re-lays the first as the second and so ties the two restatements together."""
import functools

import numpy as np

from chain_common import BEHIND, EVENT, PATH_ROW, PATH_WIDE, PILE_COL, PILE_TOTAL, QUERY_SHORT
from dtw_ref import QLENS

LONG_QMAX = 1 << 20


# ---------------------------------------------------------------------------------------------------------------- §4.18

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


# ---------------------------------------------------------------------------------------------------------------- §4.22

class LongCase:
    """the inputs of s5gpu_pileup_accum_long_dev on the host: q, lo, hi [total_rows], first [n + 1] uint64, qlen [n], status [n], ref [R],
    ev [total_rows] EVENT and ev_skip.  total_rows is the arrays' length whatever `first` claims."""

    def __init__(self, q, first, qlen, ref, lo, hi, status=None, ev=None, ev_skip=0):
        self.q = np.ascontiguousarray(q, dtype=np.int16)
        self.total = len(self.q)
        self.first = np.asarray(first, dtype=np.uint64).copy()
        self.n = len(self.first) - 1
        self.qlen = np.asarray(qlen, dtype=np.uint32).copy()
        self.ref = np.ascontiguousarray(ref, dtype=np.int16)
        self.R = len(self.ref)
        self.lo, self.hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
        self.status = np.zeros(self.n, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32).copy()
        if ev is None:
            ev = np.zeros(self.total, dtype=EVENT)
            ev["length"] = np.random.default_rng(self.n * 31 + self.R).integers(1, 5000, self.total)
            ev["start"], ev["mean"], ev["stdv"] = 7, 1.5, 0.25
        self.ev = np.ascontiguousarray(ev, dtype=EVENT)
        self.ev_skip = int(ev_skip)
        assert self.n >= 0 and len(self.qlen) == len(self.status) == self.n and len(self.lo) == len(self.hi) == len(self.ev) == self.total

    def copy(self):
        return LongCase(self.q.copy(), self.first, self.qlen, self.ref.copy(), self.lo.copy(), self.hi.copy(), self.status, self.ev.copy(), self.ev_skip)


def pileup_long_ref(case, events=True):
    """(total, cols) of §4.22 for a LongCase.  int64 numpy, a read at a time; the invariants asserted."""
    R = case.R
    r = case.ref.astype(np.int64)
    depth, n_events, n_samples = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    sum_q, sumsq_q, sum_cost = np.zeros(R, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    min_q, max_q = np.full(R, 32767, np.int64), np.full(R, -32768, np.int64)
    used = skipped = bad = cells = cost = spans = 0
    skip = case.ev_skip if events else 0
    for k in range(case.n):
        Q, f0, f1 = int(case.qlen[k]), int(case.first[k]), int(case.first[k + 1])
        if case.status[k] != 0 or Q == 0:
            skipped += 1
            continue
        if Q > LONG_QMAX or f0 > f1 or f1 > case.total or Q + skip > f1 - f0:
            bad += 1
            continue
        lo, hi = case.lo[f0:f0 + Q].astype(np.int64), case.hi[f0:f0 + Q].astype(np.int64)
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
        q = case.q[f0:f0 + Q].astype(np.int64)[i]
        c = np.abs(q - r[j])
        np.add.at(depth, j, first.astype(np.int64))
        np.add.at(n_events, j, 1)
        if events:
            np.add.at(n_samples, j, case.ev["length"][f0 + skip:f0 + skip + Q].astype(np.int64)[i])
        np.add.at(sum_q, j, q)
        np.add.at(sumsq_q, j, q * q)
        np.add.at(sum_cost, j, c)
        np.minimum.at(min_q, j, q)
        np.maximum.at(max_q, j, q)
        cells += len(j)
        cost += int(c.sum())
        spans += int(hi[Q - 1] - lo[0] + 1)
        assert int(first.sum()) == int(hi[Q - 1] - lo[0] + 1)              # a read is first once in every column it covers, seams or not
    assert int(n_events.sum()) == cells and int(sum_cost.sum()) == cost and int(depth.sum()) == spans
    assert used + skipped + bad == case.n and (depth <= n_events).all() and n_events.max(initial=0) < 2 ** 32 and sumsq_q.min(initial=0) >= 0
    cols = np.zeros(R, dtype=PILE_COL)
    for name, a in (("depth", depth), ("n_events", n_events), ("n_samples", n_samples), ("sum_q", sum_q), ("sumsq_q", sumsq_q), ("sum_cost", sum_cost),
                    ("min_q", min_q), ("max_q", max_q)):
        cols[name] = a
    total = np.zeros(1, dtype=PILE_TOTAL)
    total[0] = (used, skipped, bad, cells, cost, R, (0, 0, 0, 0, 0))
    return total[0], cols


def relay(case, ev_skip=0, seed=1):
    """a Case re-laid as ragged: read k's Q = min(qlen, pitch) rows at first[k], its event rows ev_skip further on, and 0 to 2
    rows that belong to nobody behind them"""
    rng = np.random.default_rng(seed)
    Q = np.minimum(case.qlen.astype(np.int64), case.pitch)
    rows = Q + ev_skip + rng.integers(0, 3, case.n)
    first = np.concatenate(([0], np.cumsum(rows))).astype(np.uint64)
    total = int(first[-1])
    q, lo, hi = np.zeros(total, np.int16), np.full(total, BEHIND, np.int32), np.full(total, BEHIND, np.int32)
    ev = np.zeros(total, dtype=EVENT)
    ev["length"] = 99999                                                    # (never a row's own: a wrong index shows)
    for k in range(case.n):
        f, n = int(first[k]), int(Q[k])
        q[f:f + n], lo[f:f + n], hi[f:f + n] = case.qm[k, :n], case.lo[k, :n], case.hi[k, :n]
        ev[f + ev_skip:f + ev_skip + n] = case.ev[k, :n]
    return LongCase(q, first, Q, case.ref, lo, hi, case.status, ev, ev_skip)


def path_of(start, steps, spans):
    """lo, hi of the path that starts at column `start`: row i begins steps[i] (0 or 1) right of where row i - 1 ended and covers spans[i]"""
    lo, hi = np.zeros(len(spans), np.int64), np.zeros(len(spans), np.int64)
    at = start
    for i, (st, sp) in enumerate(zip(steps, spans)):
        lo[i] = at if i == 0 else at + st
        at = hi[i] = lo[i] + sp - 1
    return lo, hi


def from_paths(seed, paths, R, ev_skip=0, lohi=127):
    """a LongCase of the reads whose (lo, hi) are given, random queries and reference"""
    rng = np.random.default_rng(seed)
    Q = np.array([len(p[0]) for p in paths], dtype=np.int64)
    first = np.concatenate(([0], np.cumsum(Q + ev_skip))).astype(np.uint64)
    total = int(first[-1])
    lo, hi = np.full(total, BEHIND, np.int32), np.full(total, BEHIND, np.int32)
    for k, (l, h) in enumerate(paths):
        f = int(first[k])
        lo[f:f + len(l)], hi[f:f + len(h)] = l, h
    return LongCase(rng.integers(-lohi, lohi + 1, total), first, Q, rng.integers(-lohi, lohi + 1, R), lo, hi, ev_skip=ev_skip)


def mixed_long(R, ev_skip=0):
    qlens = [1, 63, 64, 65, 128, 129, 1025, 3000]
    rng = np.random.default_rng(500 + R)
    lo, hi = random_paths(rng, qlens, R, 3000)
    return from_paths(600 + R, [(lo[k, :Q], hi[k, :Q]) for k, Q in enumerate(qlens)], R, ev_skip)


def seams_case():
    """at segments of 64 rows: read 0 has a row of 300 columns that ends segment 0 (row 63) and another that starts segment 1 (row 64); read 1
    stays at rows 64 and 128 (lo == hi of the row before), read 2 steps there; every read covers its columns once"""
    R, Q = 1000, 200
    ones, zeros = np.ones(Q, np.int64), np.zeros(Q, np.int64)
    sp = ones.copy()
    sp[63] = sp[64] = 300
    st = zeros.copy()
    st[64] = 1
    wide = path_of(10, st, sp)
    rng = np.random.default_rng(64)
    st1, st2, sp12 = rng.integers(0, 2, Q), rng.integers(0, 2, Q), rng.integers(1, 4, Q)
    st1[[64, 128]], st2[[64, 128]] = 0, 1
    stay, step = path_of(100, st1, sp12), path_of(120, st2, sp12)
    assert wide[1][63] - wide[0][63] + 1 == 300 and wide[0][64] == wide[1][63] + 1 and wide[1][64] - wide[0][64] + 1 == 300
    assert stay[0][64] == stay[1][63] and stay[0][128] == stay[1][127] and step[0][64] == step[1][63] + 1 and step[0][128] == step[1][127] + 1
    assert max(wide[1][-1], stay[1][-1], step[1][-1]) < R
    return from_paths(65, [wide, stay, step], R)


def flawed_long_cases():
    """{name: (LongCase, skipped, bad)}: two reads of 200 rows around a 3000-row read that is valid but for one flaw (a segment of 64 rows
    never sees a flaw in another), or that is skipped"""
    R, Q, at = 4000, 3000, 1
    rng = np.random.default_rng(3000)
    lo, hi = random_paths(rng, [200, Q, 200], R - 4, 3000, start=[5, 20, 900])
    assert hi[at, Q - 1] < R - 4
    base = from_paths(3001, [(lo[k, :n], hi[k, :n]) for k, n in enumerate([200, Q, 200])], R)
    f = int(base.first[at])
    out = {}

    def put(name, skipped, bad, fn):
        c = base.copy()
        fn(c)
        out[name] = (c, skipped, bad)
    put("valid", 0, 0, lambda c: None)
    put("lo -1 at row 2999", 0, 1, lambda c: c.lo.__setitem__(f + 2999, -1))
    put("hi R at row 0", 0, 1, lambda c: c.hi.__setitem__(f, R))

    def gap2(c):                                                            # rows 128 .. move right by 2: only the gap rule fails, at row 128
        c.lo[f + 128:f + Q] += 2
        c.hi[f + 128:f + Q] += 2
    put("gap 2 between rows 127 and 128", 0, 1, gap2)
    for s in (QUERY_SHORT, PATH_WIDE, PATH_ROW, 5):
        put("status %d" % s, 1, 0, lambda c, s=s: c.status.__setitem__(at, s))
    put("qlen 0", 1, 0, lambda c: c.qlen.__setitem__(at, 0))
    return out


def layout_cases():
    """{name: (LongCase, bad read)}: four reads of 150 rows, one of which fails ONE layout check; its own path is valid, so a missing check
    would show in the table"""
    out = {}
    R, Q = 700, 150

    def base(ev_skip=0, pad=0, qs=(Q, Q, Q, Q)):
        rng = np.random.default_rng(150)
        lo, hi = random_paths(rng, list(qs), R, max(qs))
        c = from_paths(151, [(lo[k, :n], hi[k, :n]) for k, n in enumerate(qs)], R, ev_skip)
        if pad:                                                             # rows behind the last read that belong to nobody
            c = LongCase(np.concatenate((c.q, np.zeros(pad, np.int16))), c.first, c.qlen, c.ref, np.concatenate((c.lo, np.full(pad, BEHIND, np.int32))),
                         np.concatenate((c.hi, np.full(pad, BEHIND, np.int32))), c.status, np.concatenate((c.ev, np.zeros(pad, EVENT))), ev_skip)
        return c
    # first[1] > first[2]: read 1 claims rows [200, 150); read 0 keeps its 150 rows, read 2 starts at 150 as if read 1 were empty
    c = base(qs=(Q, 0, Q, Q))
    c.first[1] = 200
    c.qlen[1] = 1                                                           # (row 200 is a row of read 2's: valid as a row 0)
    out["first[k] > first[k + 1]"] = (c, 1)
    c = base()
    c.first[4] = c.total + 1
    out["first[k + 1] > total_rows"] = (c, 3)
    c = base(ev_skip=3, pad=8)
    c.qlen[2] += 1                                                          # Q + ev_skip one above the read's rows; the row behind is made valid
    f = int(c.first[2])
    c.lo[f + Q] = c.hi[f + Q] = c.hi[f + Q - 1]
    out["Q + ev_skip one above the rows"] = (c, 2)
    # Q = 2^20 + 1 with the rows to match: a read that stays at column 3 all the way
    big = LONG_QMAX + 1
    lo, hi = random_paths(np.random.default_rng(7), [Q, Q], R, Q)
    stay = (np.full(big, 3, np.int64), np.full(big, 3, np.int64))
    c = from_paths(152, [(lo[0], hi[0]), stay, (lo[1], hi[1])], R)
    out["Q = 2^20 + 1"] = (c, 1)
    return out


def sums_long():
    """one read of 65 536 rows, every q = 32767, on a reference of one level -32768"""
    Q = 65536
    return LongCase(np.full(Q, 32767, np.int16), [0, Q], [Q], [-32768], np.zeros(Q, np.int32), np.zeros(Q, np.int32))


def piling_case():
    """48 reads of 700 rows piling on the same 300 columns"""
    rng = np.random.default_rng(48)
    n, Q = 48, 700
    lo, hi = random_paths(rng, [Q] * n, 1000, Q, start=rng.integers(100, 104, n), cap=399)
    return from_paths(49, [(lo[k], hi[k]) for k in range(n)], 1000)


@functools.lru_cache(maxsize=None)
def long_cases():
    """the case list of the CPU and the GPU tests: {name: LongCase}, at segments of 64 rows unless a test says otherwise"""
    cases = {}
    for R in (1, 65, 5000):
        cases["mixed R=%d" % R] = mixed_long(R)
    cases["mixed R=5000 ev_skip 3"] = mixed_long(5000, 3)
    cases["seams"] = seams_case()
    cases.update({"flawed: " + k: v[0] for k, v in flawed_long_cases().items()})
    cases.update({"layout: " + k: v[0] for k, v in layout_cases().items()})
    cases["64-bit sums"] = sums_long()
    cases["piling"] = piling_case()
    cases["empty batch"] = LongCase(np.zeros(0, np.int16), [0], [], [1, 2, 3], np.zeros(0, np.int32), np.zeros(0, np.int32))
    cases["n = 1"] = from_paths(1, [path_of(2, np.ones(70, np.int64), np.full(70, 2, np.int64))], 200)
    return cases


def _first_lo(case):
    at = [int(case.lo[int(case.first[k])]) for k in range(case.n) if case.status[k] == 0 and case.qlen[k] and int(case.first[k]) < case.total]
    at = [a for a in at if 0 <= a < case.R]
    return min(at) if at else 0
