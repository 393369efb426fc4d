"""The restatement of refine over whole reads (docs/codecs.md §4.24) and the cases the CPU and the GPU tests share.  Nothing of the
alignment, the fit or the tables is stated again here: band_ref is extend_ref's, fit_ref and requant_ref refine_ref's, LongCase
pileup_ref's.  What is stated here is who is fitted (§4.22's verdict with ev_skip = 0), the layout of the outputs, and the rule of the
rounds."""
import numpy as np

from chain_common import EXT_ROW, FIT, NO_COST64, PATH_ROW
from extend_ref import band_ref, planted_read, planted_share
from pileup_ref import LONG_QMAX, LongCase
from refine_ref import FIT_NONE, fit_ref, requant_ref

V_USED, V_SKIPPED, V_BAD = 0, 1, 2


def row_none(status):
    return (NO_COST64, 0, 0, -1, -1, -1, int(status))


def rows_ok_ref(lo, hi, R):
    """the row rule of §4.18 over the Q >= 1 rows of a read"""
    lo, hi = np.asarray(lo).astype(np.int64), np.asarray(hi).astype(np.int64)
    return bool(((0 <= lo) & (lo <= hi) & (hi < R)).all() and np.isin(lo[1:] - hi[:-1], (0, 1)).all())


def verdict_ref(case, k, status=None, lo=None, hi=None):
    """§4.22's verdict of read k with ev_skip = 0: skipped, bad (the layout, or any row) or used"""
    Q, f0, f1 = int(case.qlen[k]), int(case.first[k]), int(case.first[k + 1])
    st = int(case.status[k] if status is None else status[k])
    lo, hi = (case.lo if lo is None else lo), (case.hi if hi is None else hi)
    if st != 0 or Q == 0:
        return V_SKIPPED
    if Q > LONG_QMAX or f0 > f1 or f1 > case.total or Q > f1 - f0:
        return V_BAD
    return V_USED if rows_ok_ref(lo[f0:f0 + Q], hi[f0:f0 + Q], case.R) else V_BAD


def fit_long_ref(case, P, status=None, lo=None, hi=None):
    """s5gpu_path_fit_long_dev on a LongCase (its status is status_in) -> (fit [n] FIT, q' [total_rows], status [n]): the verdict, the sums in
    Python integers and the solve in np.float64 (fit_ref), q' at the rows of the reads whose status is 0 and zeros everywhere else"""
    status = case.status if status is None else status
    lo, hi = (case.lo if lo is None else lo), (case.hi if hi is None else hi)
    fit, q1, st = np.zeros(case.n, dtype=FIT), np.zeros(case.total, dtype=np.int16), np.zeros(case.n, dtype=np.int32)
    for k in range(case.n):
        v = verdict_ref(case, k, status, lo, hi)
        fit[k] = FIT_NONE
        if v != V_USED:
            st[k] = status[k] if v == V_SKIPPED else PATH_ROW
            continue
        Q, f0 = int(case.qlen[k]), int(case.first[k])
        st[k], f = fit_ref(case.q[f0:f0 + Q], case.ref, lo[f0:f0 + Q], hi[f0:f0 + Q], P)
        assert 0 < f[2] < 2 ** 20 + 2 ** 26 and all(abs(x) < 2 ** 57 for x in f[2:])
        fit[k] = f
        if st[k] == 0:
            q1[f0:f0 + Q] = requant_ref(case.q[f0:f0 + Q], f[0], f[1], P["clip"])
    return fit, q1, st


def refine_long_ref(case, rows, T, band, P, trace=None):
    """s5gpu_extend_refine_dev on a LongCase (q: the long queries that came in, lo, hi: the paths that came in; its status is not read) and the
    EXT_ROW array `rows` that came in (a read's status_in is its row's) -> dict(q, rows, lo, hi, fit, rounds).
    Round 0: copies of what came in for the reads §4.22 would use, "no result" (zeros, -1s, the empty row with the status) for the others.
    Round j >= 1, for a read that has status 0 and a query: fit_ref of the query that CAME IN along the path it has, q' = requant_ref,
    band_ref of q' from `start` of the row it has; if both succeed that is its result and rounds = j, else it keeps what it has, its row
    takes the status and it takes no further part.
    trace (a list): gets a dict per round, trace[j] for round j: `out`, `cur`: copies of the outputs and the statuses behind the round, and for
    j >= 1 what the round tried: fit (the sums also where the fit is refused), sf, t_q, t_rows, t_lo, t_hi as the fit and the band call leave
    them (a read that takes no part: no fit, its status, the empty row)."""
    n, total = case.n, case.total
    st_in = np.array([int(r["status"]) for r in rows], dtype=np.int32)
    out = dict(q=np.zeros(total, np.int16), rows=np.zeros(n, dtype=EXT_ROW), lo=np.full(total, -1, np.int32), hi=np.full(total, -1, np.int32),
               fit=np.zeros(n, dtype=FIT), rounds=np.zeros(n, np.uint32))
    cur = np.zeros(n, np.int32)
    for k in range(n):
        v = verdict_ref(case, k, st_in)
        out["fit"][k] = FIT_NONE
        if v != V_USED:
            cur[k] = st_in[k] if v == V_SKIPPED else PATH_ROW
            out["rows"][k] = row_none(cur[k])
            continue
        Q, f0 = int(case.qlen[k]), int(case.first[k])
        out["rows"][k] = rows[k]
        out["q"][f0:f0 + Q], out["lo"][f0:f0 + Q], out["hi"][f0:f0 + Q] = case.q[f0:f0 + Q], case.lo[f0:f0 + Q], case.hi[f0:f0 + Q]
    if trace is not None:
        trace.append(dict(out={key: v.copy() for key, v in out.items()}, cur=cur.copy()))
    for j in range(1, P["iters"] + 1):
        t = dict(fit=np.zeros(n, dtype=FIT), sf=cur.copy(), t_q=np.zeros(total, np.int16), t_rows=np.zeros(n, dtype=EXT_ROW),
                 t_lo=np.full(total, -1, np.int32), t_hi=np.full(total, -1, np.int32))
        for k in range(n):
            Q, f0 = int(case.qlen[k]), int(case.first[k])
            t["fit"][k] = FIT_NONE
            t["t_rows"][k] = row_none(cur[k])
            if cur[k] != 0 or Q == 0:
                continue
            s = slice(f0, f0 + Q)
            assert rows_ok_ref(out["lo"][s], out["hi"][s], case.R)         # what a round left is a path
            sf, f = fit_ref(case.q[s], case.ref, out["lo"][s], out["hi"][s], P)
            t["fit"][k], t["sf"][k] = f, sf
            st = sf
            if sf == 0:
                q1 = requant_ref(case.q[s], f[0], f[1], P["clip"])
                w = band_ref(q1, case.ref, int(out["rows"][k]["start"]), T, band)
                t["t_q"][s], t["t_rows"][k] = q1, w["row"]
                st = w["row"][6]
                if st == 0:
                    t["t_lo"][s], t["t_hi"][s] = w["lo"], w["hi"]
            else:
                t["t_rows"][k] = row_none(sf)
            if st == 0:
                out["q"][s], out["lo"][s], out["hi"][s] = t["t_q"][s], t["t_lo"][s], t["t_hi"][s]
                out["rows"][k], out["fit"][k], out["rounds"][k] = t["t_rows"][k], f, j
            else:
                cur[k] = st
                out["rows"][k]["status"] = st
        if trace is not None:
            t["out"], t["cur"] = {key: v.copy() for key, v in out.items()}, cur.copy()
            trace.append(t)
    assert (out["rows"]["status"] == cur).all()
    return out


def refined_case(case, out):
    """the LongCase that the table and the histogram are fed with behind the rounds: the refined queries, paths and statuses"""
    return LongCase(out["q"], case.first, case.qlen, case.ref, out["lo"], out["hi"], out["rows"]["status"].astype(np.int32), case.ev, case.ev_skip)


# ---------------------------------------------------------------------------------------------------------------- cases

def banded_case(qs, ref, anchors, T, band, gap=None, seed=0):
    """a LongCase and its EXT_ROW array from band_ref: read k's query qs[k] (possibly empty) aligned from anchors[k]; gap[k] rows that belong to
    nobody behind read k (default: 0 to 2, drawn from seed)"""
    rng = np.random.default_rng(seed)
    n = len(qs)
    gap = [int(x) for x in (rng.integers(0, 3, n) if gap is None else gap)]
    first = np.concatenate(([0], np.cumsum([len(q) + g for q, g in zip(qs, gap)]))).astype(np.uint64)
    total = int(first[-1])
    q, lo, hi = np.zeros(total, np.int16), np.full(total, -1, np.int32), np.full(total, -1, np.int32)
    rows = np.zeros(n, dtype=EXT_ROW)
    for k in range(n):
        f0, Q = int(first[k]), len(qs[k])
        w = band_ref(qs[k], ref, int(anchors[k]), T, band)
        rows[k] = w["row"]
        if Q and w["row"][6] == 0:
            q[f0:f0 + Q], lo[f0:f0 + Q], hi[f0:f0 + Q] = qs[k], w["lo"], w["hi"]
        elif Q:
            q[f0:f0 + Q] = qs[k]
    return LongCase(q, first, [len(x) for x in qs], ref, lo, hi, rows["status"].astype(np.int32)), rows


def planted_long(seed, n_events, R, a=0.7, b=15.0):
    """§4.24's planted case: extend_ref.planted_read, and once the read's walk is drawn the stretch of the reference it covers,
    [s - 100, last column + 100), replaced by rint(a level + b): a region whose levels sit higher and closer together than the target's
    -> (q, ref, anchor, truth)"""
    q, ref, anchor, truth = planted_read(seed, n_events, R)
    ref = ref.copy()
    s0, s1 = int(truth[0]) - 100, int(truth[-1]) + 100
    assert 0 <= s0 and s1 <= R
    ref[s0:s1] = np.rint(a * ref[s0:s1].astype(np.float64) + b).astype(np.int16)
    return q, ref, anchor, truth


def share_of(lo, hi, truth):
    """extend_ref.planted_share on arrays"""
    return planted_share(dict(lo=np.asarray(lo).astype(np.int64), hi=np.asarray(hi).astype(np.int64)), truth)[0]
