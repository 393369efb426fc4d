"""The restatements of the fold and of the estimate (docs/codecs.md §4.26) in int64 numpy and Python floats, and the cases the CPU and the
GPU tests share: fold_ref (a table of pileup folded onto classes), hist_fold_ref (a level histogram), classes_ref and levels_ref (the rank
and the level of every column of a reference made from sequences), solve_ref (the estimate), and the planted round."""
import functools
import math

import numpy as np

from chain_common import PILE_COL, PILE_TOTAL
from contrast_ref import BINS, HIST_HEAD, Q0, SHIFT, bin_of
from dtw_ref import quant_ref
from extend_ref import band_ref
from pileup_ref import LongCase, pileup_long_ref

NONE, REFUSED = 0xFFFFFFFF, 1
KMER_ROW = np.dtype([("level", "<f8"), ("stdv", "<f8"), ("dwell", "<f8"), ("cells", "<u4"), ("kept", "<u4"), ("zero", "<u8")])
SUMS = ("depth", "n_events", "n_samples", "sum_q", "sumsq_q", "sum_cost")


def empty_table(K):
    """what s5gpu_pileup_reset_dev writes for K columns"""
    total, cols = np.zeros(1, dtype=PILE_TOTAL)[0], np.zeros(K, dtype=PILE_COL)
    total["R"] = K
    cols["min_q"], cols["max_q"] = 32767, -32768
    return total, cols


def empty_hist(K, q0=Q0, shift=SHIFT):
    """what s5gpu_pile_hist_reset_dev writes for K columns"""
    head = np.zeros(1, dtype=HIST_HEAD)[0]
    head["R"], head["q0"], head["shift"], head["bins"] = K, q0, shift, BINS
    return head, np.zeros((K, BINS), dtype="<u4")


def fold_ref(table, cls, K, out=None):
    """(total, cols) of R columns added into `out` (an empty table of K columns when None) by the classes cls -> a new (total, cols).  A
    column is kept iff cls < K; an empty column adds nothing.  The invariants are asserted on an output that started empty."""
    total, cols = table
    R = len(cols)
    cls = np.asarray(cls, dtype=np.uint32)
    assert cls.shape == (R,)
    fresh = out is None
    t, c = empty_table(K) if fresh else (np.array([out[0]], dtype=PILE_TOTAL)[0], out[1].copy())
    if int(total["cells"]) >= 2 ** 32 or int(total["R"]) != R or int(t["R"]) != K:
        t["reserved"][0] |= REFUSED
        return t, c
    at = np.flatnonzero((cls < K) & (cols["n_events"] != 0))
    to = cls[at].astype(np.int64)
    for name in SUMS:
        acc = c[name].astype(np.int64 if name == "sum_q" else np.uint64)
        np.add.at(acc, to, cols[name][at].astype(acc.dtype))
        assert name not in ("depth", "n_events") or acc.max(initial=0) < 2 ** 32
        c[name] = acc
    lo, hi = c["min_q"].copy(), c["max_q"].copy()
    np.minimum.at(lo, to, cols["min_q"][at])
    np.maximum.at(hi, to, cols["max_q"][at])
    c["min_q"], c["max_q"] = lo, hi
    for name in ("reads_used", "reads_skipped", "reads_bad"):
        t[name] += total[name]
    t["cells"] += int(cols["n_events"][at].astype(np.int64).sum())
    t["cost"] += int(cols["sum_cost"][at].astype(np.uint64).sum())
    if fresh:
        assert int(c["n_events"].astype(np.int64).sum()) == int(t["cells"]) and int(c["sum_cost"].astype(np.uint64).sum()) == int(t["cost"])
        none = c["n_events"] == 0                                          # a class nothing was added to keeps the empty pair
        assert (c["min_q"][none] == 32767).all() and (c["max_q"][none] == -32768).all() and (c["min_q"][~none] <= c["max_q"][~none]).all()
    return t, c


def hist_fold_ref(hist, cls, K, out=None):
    """(head, counts [R, 64]) added into `out` (an empty histogram of K columns with the input's q0 and shift when None)"""
    head, counts = hist
    R = len(counts)
    cls = np.asarray(cls, dtype=np.uint32)
    fresh = out is None
    h, c = empty_hist(K, int(head["q0"]), int(head["shift"])) if fresh else (np.array([out[0]], dtype=HIST_HEAD)[0], out[1].copy())
    same = all(int(head[f]) == int(h[f]) for f in ("q0", "shift")) and int(head["bins"]) == BINS and int(h["bins"]) == BINS
    if int(head["cells"]) >= 2 ** 32 or int(head["R"]) != R or int(h["R"]) != K or not same:
        h["reserved"][0] |= REFUSED
        return h, c
    at = np.flatnonzero(cls < K)
    acc = c.astype(np.int64)
    np.add.at(acc, cls[at].astype(np.int64), counts[at].astype(np.int64))
    assert acc.max(initial=0) < 2 ** 32
    for name in ("reads_used", "reads_skipped", "reads_bad"):
        h[name] += head[name]
    h["cells"] += int(counts[at].astype(np.int64).sum())
    if fresh:
        assert int(acc.sum()) == int(h["cells"])
    return h, acc.astype("<u4")


def table_bytes_of(t):
    return np.array([t[0]]).tobytes() + np.ascontiguousarray(t[1]).tobytes()


# ---------------------------------------------------------------------------------------------------------------- classes and levels

def _codes(seq):
    return np.array(["ACGT".find(ch) for ch in seq.upper().replace("U", "T")], dtype=np.int64)


def _ranks(codes, k):
    """the rank of the k-mer at every start of codes, NONE where it holds a code of -1"""
    Lk = len(codes) - k + 1
    out = np.zeros(Lk, dtype=np.int64)
    bad = np.zeros(Lk, dtype=bool)
    for b in range(k):
        c = codes[b:b + Lk]
        out = out * 4 + np.maximum(c, 0)
        bad |= c < 0
    return np.where(bad, NONE, out).astype(np.uint32)


def wall_of(clip):
    return (2048 * clip) // (32768 - clip) + 1


def classes_ref(contigs, k, strands=2, rna=False, clip=127):
    """[(name, sequence)] -> (cls [R] uint32, K): the rank of the k-mer every column of the reference of §4.19 shows: per contig of k or more
    bases the forward k-mers, then (strands = 2) the k-mers of the reverse-complement sequence; rna: one segment, the columns reversed, the
    ranks not; NONE on the walls between segments and where a k-mer holds a letter other than ACGT"""
    segs = []
    for _, seq in contigs:
        if len(seq) < k:
            continue
        codes = _codes(seq)
        fwd = _ranks(codes, k)
        segs.append(fwd[::-1] if rna else fwd)
        if not rna and strands == 2:
            segs.append(_ranks(np.where(codes[::-1] < 0, -1, 3 - codes[::-1]), k))
    out = []
    for s, seg in enumerate(segs):
        if s:
            out.append(np.full(wall_of(clip), NONE, dtype=np.uint32))
        out.append(seg)
    return np.concatenate(out), 4 ** k


def levels_ref(cls, levels):
    """the float32 levels of the columns that are no wall, in order: the model's, or the table's mean (the double sum in rank order, divided,
    rounded to float) -- wall: whether a NONE column is a wall cannot be read from cls, so the caller passes the columns of the segments only"""
    lv = np.asarray(levels, dtype=np.float32)
    mean = np.float32(np.cumsum(lv.astype(np.float64))[-1] / np.float64(len(lv)))
    return np.where(cls == NONE, mean, lv[np.minimum(cls, len(lv) - 1)]).astype(np.float32)


def quant_stats_ref(m):
    """mu and sd as quant takes them: float64, strictly left to right"""
    d = np.asarray(m, dtype=np.float32).astype(np.float64)
    mu = np.cumsum(d)[-1] / np.float64(len(d))
    e = d - mu
    return float(mu), float(np.sqrt(np.cumsum(e * e)[-1] / np.float64(len(d))))


# ---------------------------------------------------------------------------------------------------------------- the estimate

def solve_ref(cols, mu, sd, scale, levels_in, min_cells=30):
    """the rows of s5gpu_kmer_model_solve from the folded columns, in Python floats (IEEE double, one operation at a time)"""
    rows = np.zeros(len(cols), dtype=KMER_ROW)
    unit = float(sd) / float(scale)
    for c in range(len(cols)):
        n = int(cols["n_events"][c])
        if n == 0 or n < min_cells:
            rows[c] = (float(np.float32(levels_in[c])), 0.0, 0.0, n, 1, 0)
            continue
        mean_q = float(int(cols["sum_q"][c])) / float(n)
        msq = float(int(cols["sumsq_q"][c])) / float(n)
        var = msq - mean_q * mean_q
        var = var if var > 0.0 else 0.0
        rows[c] = (float(mu) + unit * mean_q, unit * math.sqrt(var), float(int(cols["n_samples"][c])) / float(n), n, 0, 0)
    return rows


# ---------------------------------------------------------------------------------------------------------------- the cases

def random_table(rng, R, empty_share=0.2, extreme=False, q0=Q0, shift=SHIFT):
    """a table and a histogram of R columns with random content that keeps the invariants: cells = sum n_events, cost = sum sum_cost, the
    bins of a column add up to its n_events.  extreme: columns that hold q = -32768 and 32767"""
    total, cols = empty_table(R)
    head, counts = empty_hist(R, q0, shift)
    for j in range(R):
        if rng.random() < empty_share:
            continue
        n = int(rng.integers(1, 40))
        q = rng.integers(-127, 128, n).astype(np.int64)
        if extreme and j % 3 == 0:
            q[0] = -32768
            q[-1] = 32767
        cols[j] = (int(rng.integers(1, n + 1)), n, int(rng.integers(0, 5000 * n)), int(q.sum()), int((q * q).sum()), int(rng.integers(0, 300 * n)), int(q.min()), int(q.max()))
        np.add.at(counts[j], bin_of(q, q0, shift), 1)
    total["reads_used"], total["reads_skipped"], total["reads_bad"] = 7 + R, 3, 1
    total["cells"], total["cost"] = int(cols["n_events"].astype(np.int64).sum()), int(cols["sum_cost"].astype(np.uint64).sum())
    head["cells"], head["reads_used"], head["reads_skipped"], head["reads_bad"] = total["cells"], total["reads_used"], total["reads_skipped"], total["reads_bad"]
    return (total, cols), (head, counts)


RS = [1, 63, 64, 65, 257, 1025]
KS = [1, 4, 1024, 1025, 4096]            # 1024: the last that takes LDS


@functools.lru_cache(maxsize=None)
def fold_cases():
    """{name: (table, hist, cls, K)} over every R and K, the class maps and contents of §4.26's tests:
    one     all columns in one class (the last);           none  every class NONE
    mixed   NONE, classes >= K and empty columns interleaved with full ones, random classes
    extreme columns holding q = -32768 and 32767;           lonely  a class met only by empty columns: it keeps the empty pair"""
    out = {}
    for R in RS:
        for K in KS:
            rng = np.random.default_rng(1000 * R + K)
            table, hist = random_table(rng, R)
            out["one R=%d K=%d" % (R, K)] = (table, hist, np.full(R, K - 1, dtype=np.uint32), K)
            out["none R=%d K=%d" % (R, K)] = (table, hist, np.full(R, NONE, dtype=np.uint32), K)
            cls = rng.integers(0, K, R).astype(np.uint32)
            drop = rng.random(R)
            cls = np.where(drop < 0.15, NONE, np.where(drop < 0.3, K + rng.integers(0, 5, R), cls)).astype(np.uint32)
            out["mixed R=%d K=%d" % (R, K)] = (table, hist, cls, K)
            out["extreme R=%d K=%d" % (R, K)] = random_table(rng, R, 0.1, True) + (rng.integers(0, K, R).astype(np.uint32), K)
            if K >= 4 and R >= 63:
                t, h = random_table(rng, R, 0.0)
                c = rng.integers(1, K, R).astype(np.uint32)               # class 0: met by the empty columns only
                for j in range(0, R, 5):
                    t[1][j] = empty_table(1)[1][0]
                    h[1][j] = 0
                    c[j] = 0
                t[0]["cells"] = h[0]["cells"] = int(t[1]["n_events"].astype(np.int64).sum())
                t[0]["cost"] = int(t[1]["sum_cost"].astype(np.uint64).sum())
                out["lonely R=%d K=%d" % (R, K)] = (t, h, c, K)
    return out


# ---------------------------------------------------------------------------------------------------------------- the planted round

PLANTED_K, PLANTED_BASES, PLANTED_READS, PLANTED_EVENTS = 3, 3000, 24, 1500


@functools.lru_cache(maxsize=None)
def planted_round(seed=2600, min_cells=30):
    """One round of the estimate, wholly on the restatements.  k = 3, one seeded contig of 3000 bases (forward strand), table A with levels
    90 + N(0, 12); the truth is A + N(0, 3) per k-mer.  24 reads of 1500 events, generated as contrast_ref.planted generates its reads,
    from the truth's levels put into the reference's units ((level - mu) / sd * scale, unrounded), are aligned by band_ref against the
    reference made from A; pileup_long_ref, fold_ref, solve_ref -> dict(A, truth, rows, cls, table, folded, mu, sd)"""
    rng = np.random.default_rng(seed)
    K = 4 ** PLANTED_K
    seq = "".join("ACGT"[b] for b in rng.integers(0, 4, PLANTED_BASES))
    A = (90.0 + rng.normal(0.0, 12.0, K)).astype(np.float32)
    truth = A.astype(np.float64) + rng.normal(0.0, 3.0, K)
    cls, _ = classes_ref([("c", seq)], PLANTED_K, strands=1)
    lev = levels_ref(cls, A)
    ref = quant_ref(lev)
    mu, sd = quant_stats_ref(lev)
    lev_truth = (truth[cls] - mu) / sd * 32.0                              # the truth's levels, column by column, in the reference's units
    reads, paths = [], []
    for k in range(PLANTED_READS):
        s = int(rng.integers(64, 201))
        cols_of, col = [], s
        while len(cols_of) < PLANTED_EVENTS:
            if rng.random() >= 0.05:
                cols_of += [col] * int(rng.integers(1, 3))
            col += 1
        cols_of = np.array(cols_of[:PLANTED_EVENTS])
        q = quant_ref(1.7 * lev_truth[cols_of] + 30.0 + rng.normal(0.0, 1.5, PLANTED_EVENTS))
        w = band_ref(q, ref, s + (7 if k % 2 else -7), 64, 128)
        assert w["row"][6] == 0
        reads.append(q)
        paths.append((np.asarray(w["lo"], np.int32), np.asarray(w["hi"], np.int32)))
    Q = [len(q) for q in reads]
    first = np.concatenate(([0], np.cumsum(Q))).astype(np.uint64)
    case = LongCase(np.concatenate(reads), first, Q, ref, np.concatenate([p[0] for p in paths]), np.concatenate([p[1] for p in paths]))
    table = pileup_long_ref(case)
    folded = fold_ref(table, cls, K)
    rows = solve_ref(folded[1], mu, sd, 32.0, A, min_cells)
    return dict(A=A, truth=truth, rows=rows, cls=cls, table=table, folded=folded, mu=mu, sd=sd, seq=seq, ref=ref)
