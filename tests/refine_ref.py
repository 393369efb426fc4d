"""The restatement of refine (docs/codecs.md §4.20): the fit in Python integers and np.float64 in the order §4.20 states (fit_ref), the
requantiser (requant_ref), the realign as dtw_ref.path_ref on the slice of the reference that is the window (window_ref), the rounds
(refine_ref), and the planted case."""
import struct

import numpy as np

from chain_common import EMPTY, FIT_FLAT, FIT_RANGE, PATH_ROW, PATH_WIDE
from dtw_ref import path_ref, quant_ref

# a_min, a_max, b_max, clip, pad, min_cells, iters
DEFAULTS = dict(a_min=0.5, a_max=2.0, b_max=64.0, clip=127, pad=16, min_cells=16, iters=2)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_bytes(p):
    return struct.pack("<dddiIII", p["a_min"], p["a_max"], p["b_max"], p["clip"], p["pad"], p["min_cells"], p["iters"])


def c_params(p):
    from slow5tools_amd import _lib

    return _lib.RefineParams(p["a_min"], p["a_max"], p["b_max"], p["clip"], p["pad"], p["min_cells"], p["iters"])


# ---------------------------------------------------------------------------------------------------------------- the restatement

FIT_NONE = (1.0, 0.0, 0, 0, 0, 0, 0, 0)


def path_status_ref(lo, hi, R, wmax):
    """the row rules of §4.18 and the span of §4.20 for a path of Q >= 1 rows -> 0, PATH_ROW or PATH_WIDE"""
    lo, hi = [int(x) for x in lo], [int(x) for x in hi]
    for i in range(len(lo)):
        if lo[i] < 0 or lo[i] > hi[i] or hi[i] >= R or (i and lo[i] - hi[i - 1] not in (0, 1)):
            return PATH_ROW
    return PATH_WIDE if hi[-1] - lo[0] + 1 > wmax else 0


def fit_ref(q, r, lo, hi, P):
    """the six sums in Python integers over the cells of a valid path, and the solve in np.float64: every operation on its own, the products
    before the subtraction -> (status, (a, b, n, Sq, Sr, Sqq, Sqr, Srr))"""
    n = Sq = Sr = Sqq = Sqr = Srr = 0
    for i in range(len(q)):
        qi = int(q[i])
        seg = [int(x) for x in r[int(lo[i]):int(hi[i]) + 1]]
        n += len(seg); Sq += len(seg) * qi; Sqq += len(seg) * qi * qi
        Sr += sum(seg); Sqr += qi * sum(seg); Srr += sum(x * x for x in seg)
    sums = (n, Sq, Sr, Sqq, Sqr, Srr)
    f = np.float64
    with np.errstate(all="ignore"):
        den = f(n) * f(Sqq) - f(Sq) * f(Sq)
        if n < P["min_cells"] or not den > 0.0:
            return FIT_FLAT, (1.0, 0.0) + sums
        a = (f(n) * f(Sqr) - f(Sq) * f(Sr)) / den
        b = (f(Sr) - a * f(Sq)) / f(n)
    if not (np.isfinite(a) and P["a_min"] <= a <= P["a_max"] and abs(b) <= P["b_max"]):
        return FIT_RANGE, (1.0, 0.0) + sums
    return 0, (float(a), float(b)) + sums


def requant_ref(q0, a, b, clip):
    p = np.float64(a) * np.asarray(q0).astype(np.float64)
    s = p + np.float64(b)
    return np.clip(np.rint(s), -clip, clip).astype(np.int16)


def window_ref(q, r, row, pad, wmax):
    """§4.20's window: -> (status, row', lo, hi) of a query of Q >= 1 rows; the alignment is path_ref on the slice"""
    Q, R = len(q), len(r)
    cost, qlen, start, end = (int(x) for x in row)
    none = (EMPTY, np.full(Q, -1, dtype=np.int32), np.full(Q, -1, dtype=np.int32))
    if qlen != Q or start < 0 or start > end or end >= R:
        return (PATH_ROW,) + none
    ws, we = max(0, start - pad), min(R - 1, end + pad)
    if we - ws + 1 > wmax:
        return (PATH_WIDE,) + none
    c, lo, hi = path_ref(q, np.asarray(r)[ws:we + 1], cross_check=False)
    return 0, (c, Q, int(lo[0]) + ws, int(hi[-1]) + ws), lo + ws, hi + ws


def round_ref(q0, r, row, lo, hi, wmax, P):
    """one round for a read with a query and status 0 -> (st_fit, fit, q', st_win, row', lo', hi')"""
    Q = len(q0)
    none = (EMPTY, np.full(Q, -1, dtype=np.int32), np.full(Q, -1, dtype=np.int32))
    st = path_status_ref(lo, hi, len(r), wmax)
    if st:
        return (st, FIT_NONE, np.zeros(Q, dtype=np.int16), st) + none
    st, fit = fit_ref(q0, r, lo, hi, P)
    q1 = requant_ref(q0, fit[0], fit[1], P["clip"]) if st == 0 else np.asarray(q0, dtype=np.int16).copy()
    return (st, fit, q1) + window_ref(q1, r, row, P["pad"], wmax)


def refine_ref(q0, r, row, lo, hi, status_in, wmax, P):
    """§4.20's rounds for one read (q0: its Q rows) -> dict(q, row, lo, hi, fit, status, rounds)"""
    Q = len(q0)

    def none(st):
        return dict(q=np.zeros(Q, dtype=np.int16), row=EMPTY, lo=np.full(Q, -1, dtype=np.int32), hi=np.full(Q, -1, dtype=np.int32), fit=FIT_NONE, status=st, rounds=0)
    if status_in != 0 or Q == 0:
        return none(status_in)
    cur = dict(q=np.asarray(q0, dtype=np.int16).copy(), row=tuple(int(x) for x in row), lo=np.asarray(lo, dtype=np.int32).copy(),
               hi=np.asarray(hi, dtype=np.int32).copy(), fit=FIT_NONE, status=0, rounds=0)
    for k in range(1, P["iters"] + 1):
        sf, fit, q1, sw, row1, lo1, hi1 = round_ref(q0, r, cur["row"], cur["lo"], cur["hi"], wmax, P)
        if sf in (PATH_ROW, PATH_WIDE):
            return none(sf)
        if sf or sw:
            cur["status"] = sf or sw
            break
        cur = dict(q=q1, row=row1, lo=lo1, hi=hi1, fit=fit, status=0, rounds=k)
    return cur


def planted(seed, n_reads=24):
    """the case of §4.20: a reference of 600 levels whose halves are drawn from N(90, 12) and N(108, 20), quantised as a whole; queries of
    40 .. 129 events cut from it, put through 1.7 x + 30 plus N(0, 1) and quantised each on its own -> (ref, [(query, true_start, true_end)])"""
    rng = np.random.default_rng(seed)
    levels = np.concatenate([rng.normal(90.0, 12.0, 300), rng.normal(108.0, 20.0, 300)]).astype(np.float32)
    ref = quant_ref(levels)
    reads = []
    for _ in range(n_reads):
        Q = int(rng.integers(40, 130))
        s = int(rng.integers(0, 600 - Q + 1))
        x = 1.7 * levels[s:s + Q].astype(np.float64) + 30.0 + rng.normal(0.0, 1.0, Q)
        reads.append((quant_ref(x.astype(np.float32)), s, s + Q - 1))
    return ref, reads


def planted_refined(seed, P=None, wmax=1 << 20):
    """-> (ref, [(query, true span, first (cost, lo, hi), refine_ref's dict)])"""
    P = P or params()
    ref, reads = planted(seed)
    out = []
    for q, s, e in reads:
        c, lo, hi = path_ref(q, ref, cross_check=False)
        out.append((q, (s, e), (c, lo, hi), refine_ref(q, ref, (c, len(q), int(lo[0]), int(hi[-1])), lo, hi, 0, wmax, P)))
    return ref, out
