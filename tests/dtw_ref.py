"""The restatements of docs/codecs.md §4.16 (the quantiser and subsequence DTW) and §4.17 (the path) in numpy, and what the tests of map,
align, pileup, refine and extend share around them: the known-answer case, the lane-height rule, the query batches and map's lines."""
import numpy as np
import pytest

from chain_common import EMPTY, KNOWN_SEED, MAP_ROW

QLENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 1024]      # every lane height, both sides of every lane boundary
RS = [1, 2, 63, 64, 65, 129, 500]                                                     # R < 64, R < Q, R no multiple of the reference block


# ---------------------------------------------------------------------------------------------------------------- the restatement

def quant_ref(m, scale=32.0, clip=127):
    """quant of §4.16: float64, sums strictly left to right (cumsum accumulates in order; np.sum would add pairwise)"""
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
    """(cost, start, end) of §4.16 for a batch q[B, Q] of queries of one length (or one query q[Q]) against r[R]: int64 matrices D and S
    filled along anti-diagonals, the predecessor of least D with ties to the diagonal, then (i - 1, j), then (i, j - 1)"""
    q = np.asarray(q).astype(np.int64)
    one = q.ndim == 1
    if one:
        q = q[None, :]
    r = np.asarray(r).astype(np.int64)
    B, Q = q.shape
    R = len(r)
    assert Q >= 1 and R >= 1
    INF = np.int64(1) << 40
    D = np.full((B, Q + 1, R + 1), INF, dtype=np.int64)                    # D[:, i + 1, j + 1] is D[i][j]; row 0: "a path starts here"
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
    end = np.argmin(last, axis=1)                                          # the first of equal minima: the smallest j
    b = np.arange(B)
    cost, start = last[b, end], S[b, Q, end + 1]
    return (int(cost[0]), int(start[0]), int(end[0])) if one else (cost, start, end)


def rows_ref(queries, qlens, r, want_start):
    """the MAP_ROW rows of a batch: queries a list of int16 arrays (or a matrix), qlens what of each is the query"""
    out = np.zeros(len(qlens), dtype=MAP_ROW)
    for i, n in enumerate(qlens):
        if n == 0:
            out[i] = EMPTY
        else:
            c, s, e = sdtw_ref(np.asarray(queries[i])[:n], r)
            out[i] = (c, n, s if want_start else -1, e)
    return out


def path_ref(q, r, cross_check=True):
    """(cost, lo, hi) of §4.17 for ONE query: the full D in int64, filled along anti-diagonals; the walk from
    (Q - 1, end) takes the predecessor of least D, ties to the diagonal, then (i - 1, j), then (i, j - 1), until row 0.  The three invariants
    are asserted, and sdtw_ref with cross_check."""
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
    if cross_check:
        assert sdtw_ref(q, r) == (cost, int(lo[0]), end)
    return cost, lo.astype(np.int32), hi.astype(np.int32)


def known_answer_cases(n_draws=40):
    """§4.16's known answer: a reference of 1200 levels from -100 .. 100, neighbours at least 20 apart; a query that is the slice [a, a + Q)
    with every level but the first and the last held 1 to 3 times (time warping) aligns at cost 0 from a to a + Q - 1.  Draws whose level
    sequence stands in the reference twice are dropped.  -> (ref, [(query, a, Q, rep)]), rep the times each level is held"""
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


# ---------------------------------------------------------------------------------------------------------------- batches

def _g_of(Q):
    """the lane height: the rows of a query of Q that one of the 64 lanes holds"""
    return next(g for g in (1, 2, 4, 8, 16) if 64 * g >= Q)


def _mixed(rng, lo, hi):
    """the mixed batch: a [16, 1024] matrix with row i random in [lo, hi] up to QLENS[i]; behind the query stands what a kernel must not read
    as part of it"""
    qm = np.full((len(QLENS), 1024), 9999, dtype=np.int16)
    for i, n in enumerate(QLENS):
        qm[i, :n] = rng.integers(lo, hi + 1, n)
    return qm


@pytest.fixture(scope="module")
def mixed_batches():
    rng = np.random.default_rng(4)
    return {"pm127": _mixed(rng, -127, 127), "ties": _mixed(rng, -1, 1)}


def last_lane_batch(seed=41):
    """Every row of the last lane: for each lane height G the queries of Q = 64 G - k rows, k < G, whose last row is row (Q - 1) % G of the
    lane that holds it (the walks are compiled per such row), and for G > 1 the smallest query of the class, 32 G + 1.  -> (the [35, 1024]
    matrix of +-127, 9999 behind each query; the 35 lengths).  That every row of every lane height occurs is asserted here."""
    ql = [64 * g - k for g in (1, 2, 4, 8, 16) for k in range(g)] + [32 * g + 1 for g in (2, 4, 8, 16)]
    for g in (1, 2, 4, 8, 16):
        assert {(Q - 1) % g for Q in ql if _g_of(Q) == g} == set(range(g)), g
    rng = np.random.default_rng(seed)
    qm = np.full((len(ql), 1024), 9999, dtype=np.int16)
    for i, n in enumerate(ql):
        qm[i, :n] = rng.integers(-127, 128, n)
    return qm, ql


@pytest.fixture(scope="module")
def map_ref():
    rng = np.random.default_rng(21)
    return quant_ref(rng.normal(90.0, 12.0, 800).astype(np.float32))


def map_lines(ids, rows, want_start):
    """s5map's lines, formatted from MAP_ROW rows"""
    out = []
    for rid, r in zip(ids, rows):
        if r["qlen"] == 0:
            out.append(rid + b"\t*\t*\t*\t*\t*\n")
        else:
            out.append(b"%s\t%d\t%d\t%s\t%s\t%d\n" % (rid, r["qlen"], r["cost"], b"%.6g" % (float(r["cost"]) / float(r["qlen"])),
                                                     b"%d" % r["start"] if want_start else b"*", r["end"]))
    return b"".join(out)
