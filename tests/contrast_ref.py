"""The restatements of contrast (docs/codecs.md §4.23) in Python integers and int64 numpy, and the cases the CPU and the GPU tests share:
hist_ref (the histogram of a pileup_ref.LongCase), contrast_ref (the rows of two histograms), and the planted case."""
import functools
from fractions import Fraction

import numpy as np

from dtw_ref import quant_ref
from extend_ref import band_ref
from pileup_ref import LONG_QMAX, LongCase, from_paths, long_cases, path_of, pileup_long_ref

HIST_HEAD = np.dtype([("cells", "<u8"), ("reads_used", "<u8"), ("reads_skipped", "<u8"), ("reads_bad", "<u8"), ("R", "<u4"), ("q0", "<i4"), ("shift", "<u4"),
                      ("bins", "<u4"), ("reserved", "<u8", (2,))])
CONTRAST_ROW = np.dtype([("n_a", "<u4"), ("n_b", "<u4"), ("depth_a", "<u4"), ("depth_b", "<u4"), ("ks_num", "<u8"), ("ov_num", "<u8"), ("ks_bin", "<u2"),
                         ("med_a", "<u2"), ("med_b", "<u2"), ("flags", "<u2")])
BINS, Q0, SHIFT = 64, -128, 2


def bin_of(q, q0, shift):
    d = np.asarray(q).astype(np.int64) - q0
    return np.where(d < 0, 0, np.minimum(d >> shift, BINS - 1))


def hist_ref(case, q0=Q0, shift=SHIFT):
    """(head, counts [R, 64]) of §4.23 for a LongCase: the verdicts and cells of §4.22 without events; the invariants against
    pileup_long_ref of the same case asserted"""
    R = case.R
    counts = np.zeros((R, BINS), np.int64)
    used = skipped = bad = cells = 0
    for k in range(case.n):
        Q, f0, f1 = int(case.qlen[k]), int(case.first[k]), int(case.first[k + 1])
        if case.status[k] != 0 or Q == 0:
            skipped += 1
            continue
        if Q > LONG_QMAX or f0 > f1 or f1 > case.total or Q > f1 - f0:
            bad += 1
            continue
        lo, hi = case.lo[f0:f0 + Q].astype(np.int64), case.hi[f0:f0 + Q].astype(np.int64)
        if not (((0 <= lo) & (lo <= hi) & (hi < R)).all() and bool(np.isin(lo[1:] - hi[:-1], (0, 1)).all())):
            bad += 1
            continue
        used += 1
        w = hi - lo + 1
        i = np.repeat(np.arange(Q), w)
        j = lo[i] + np.arange(w.sum()) - np.repeat(np.cumsum(w) - w, w)
        np.add.at(counts, (j, bin_of(case.q[f0:f0 + Q], q0, shift)[i]), 1)
        cells += len(j)
    total, cols = pileup_long_ref(case, events=False)
    assert counts.sum(axis=1).tolist() == cols["n_events"].tolist() and counts.max(initial=0) < 2 ** 32
    assert (cells, used, skipped, bad) == (total["cells"], total["reads_used"], total["reads_skipped"], total["reads_bad"]) and int(counts.sum()) == cells
    head = np.zeros(1, dtype=HIST_HEAD)
    head[0] = (cells, used, skipped, bad, R, q0, shift, BINS, (0, 0))
    return head[0], counts.astype("<u4")


def hist_bytes_of(h):
    return np.array([h[0]]).tobytes() + np.ascontiguousarray(h[1], dtype="<u4").tobytes()


def contrast_ref(A, B, acc_a=None, acc_b=None, heads_agree=True):
    """the rows of §4.23 for two [R, 64] count arrays and, when given, the two tables' columns (PILE_COL arrays), in Python integers"""
    R = len(A)
    rows = np.zeros(R, dtype=CONTRAST_ROW)
    if not heads_agree:
        rows["flags"] = 128
        return rows
    for j in range(R):
        a, b = [int(x) for x in A[j]], [int(x) for x in B[j]]
        ca, cb = np.cumsum(np.array(a, dtype=object)).tolist(), np.cumsum(np.array(b, dtype=object)).tolist()
        na, nb = ca[-1], cb[-1]
        flags = (1 if na == 0 else 0) | (2 if nb == 0 else 0)
        ks = ov = ks_bin = 0
        if na >= 2 ** 31 or nb >= 2 ** 31:
            flags |= 8
        else:
            d = [abs(ca[x] * nb - cb[x] * na) for x in range(BINS)]
            ks = max(d)
            ks_bin = d.index(ks)
            assert ks < 2 ** 62 and 0 <= ks <= na * nb
            if ca[ks_bin] * nb > cb[ks_bin] * na:
                flags |= 4
            ov = sum(min(a[x] * nb, b[x] * na) for x in range(BINS))
            assert 0 <= ov <= na * nb
        med_a = next(x for x in range(BINS) if 2 * ca[x] >= na)
        med_b = next(x for x in range(BINS) if 2 * cb[x] >= nb)
        da = db = 0
        if acc_a is not None:
            da, db = int(acc_a["depth"][j]), int(acc_b["depth"][j])
            flags |= (16 if int(acc_a["n_events"][j]) != na else 0) | (32 if int(acc_b["n_events"][j]) != nb else 0)
        rows[j] = (min(na, 2 ** 32 - 1), min(nb, 2 ** 32 - 1), da, db, ks, ov, ks_bin, med_a, med_b, flags)
    return rows


# ---------------------------------------------------------------------------------------------------------------- the cases

def edge_levels(q0, shift):
    """the levels at the bin rule's edges, inside int16"""
    v = [q0 - 1, q0, q0 + (64 << shift) - 1, q0 + (64 << shift), -32768, 32767, q0 + (1 << shift) - 1, q0 + (1 << shift), q0 + (63 << shift) - 1, q0 + (63 << shift)]
    return np.clip(np.array(v, dtype=np.int64), -32768, 32767).astype(np.int16)


def edge_case(R, seed=7):
    """The smallest shapes at which the kernel can go wrong, on R columns (R = 1: every path stays on column 0): a read of 1 row on 1 column;
    a read of 65 rows with a row spanning min(70, R) columns; a read of 257 rows that ends on the table's last column; 64 reads of 3 rows on
    the same 3 columns; a read of 257 rows that is bad in its last row; a skipped read and one without a query"""
    rng = np.random.default_rng(seed + R)
    one = np.ones(1, np.int64)

    def walk(start, Q, wide_at=None, wide=1):
        """a random walk from `start`, clamped to the table (a clamped path stays on the last column: still valid)"""
        sp = np.ones(Q, np.int64)
        if wide_at is not None:
            sp[wide_at] = wide
        lo, hi = path_of(start, rng.integers(0, 2, Q), sp)
        return np.minimum(lo, R - 1), np.minimum(hi, R - 1)
    paths = [path_of(0, one, one)]
    paths.append(walk(0, 65, 30, min(70, R)))
    paths.append(walk(max(R - 40, 0), 257))                                 # ... ends on the last column
    c0 = min(40, max(R - 3, 0))
    for _ in range(64):
        paths.append(path_of(c0, np.ones(3, np.int64), np.ones(3, np.int64)) if R >= 3 else path_of(0, np.zeros(3, np.int64), np.ones(3, np.int64)))
    paths.append(walk(min(5, R - 1), 257))                                  # made bad below
    paths.append(walk(0, 10))                                               # skipped
    paths.append(walk(0, 10))                                               # qlen 0
    c = from_paths(seed, paths, R)
    n = len(paths)
    c.lo[int(c.first[n - 3]) + 256] = -1
    c.status[n - 2] = 5
    c.qlen[n - 1] = 0
    assert int(c.hi[int(c.first[2]) + 256]) == R - 1
    return c


def with_levels(case, q0, shift, seed=11):
    """the case with its queries drawn from the bin rule's edges and from around the bins"""
    c = case.copy()
    rng = np.random.default_rng(seed)
    e = edge_levels(q0, shift)
    spread = np.clip(q0 + rng.integers(-(8 << shift), (72 << shift) + 1, c.total), -32768, 32767).astype(np.int16)
    c.q = np.where(rng.random(c.total) < 0.3, e[rng.integers(0, len(e), c.total)], spread).astype(np.int16)
    return c


BIN_PARAMS = [(Q0, SHIFT), (0, 0), (-32768, 10), (32767, 0), (-300, 3)]


@functools.lru_cache(maxsize=None)
def hist_cases():
    """{name: (LongCase, q0, shift)}: the hand-made cases at every bin rule, and the case list of test_pileup_long at the default bins"""
    out = {}
    for R in (1, 65, 300):
        for q0, shift in BIN_PARAMS if R == 300 else BIN_PARAMS[:2]:
            out["edges R=%d q0=%d shift=%d" % (R, q0, shift)] = (with_levels(edge_case(R), q0, shift), q0, shift)
    for name, c in long_cases().items():
        out[name] = (c, Q0, SHIFT)
    return out


_WANT = {}


def wanted(name):
    if name not in _WANT:
        c, q0, shift = hist_cases()[name]
        _WANT[name] = hist_bytes_of(hist_ref(c, q0, shift))
    return _WANT[name]


# ---------------------------------------------------------------------------------------------------------------- the planted case

PLANTED_R, PLANTED_READS, PLANTED_EVENTS, PLANTED_COLS, PLANTED_SHIFT = 2048, 12, 1500, (700, 709), 48.0


@functools.lru_cache(maxsize=None)
def planted(seed=2300):
    """-> (ref, sides): ref the 2048 levels; sides[s] a list of 12 (q, anchor) pairs, the reads generated as extend_ref.planted_read
    generates them from a start in columns 64 .. 200; side 1 has 48 added to the levels of columns 700 .. 709 before the quantiser"""
    rng = np.random.default_rng(seed)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, PLANTED_R)), -127, 127).astype(np.int16)
    sides = []
    for side in range(2):
        lev = ref.astype(np.float64)
        if side:
            lev[PLANTED_COLS[0]:PLANTED_COLS[1] + 1] += PLANTED_SHIFT
        reads = []
        for k in range(PLANTED_READS):
            s = int(rng.integers(64, 201))
            truth, col = [], s
            while len(truth) < PLANTED_EVENTS:
                if rng.random() >= 0.05:
                    truth += [col] * int(rng.integers(1, 3))
                col += 1
            truth = np.array(truth[:PLANTED_EVENTS])
            q = quant_ref(1.7 * lev[truth] + 30.0 + rng.normal(0.0, 1.5, PLANTED_EVENTS))
            reads.append((q, s + (7 if k % 2 else -7)))
        sides.append(reads)
    return ref, sides


def planted_case(ref, reads, paths):
    """a LongCase of one side's reads with the (lo, hi) given"""
    Q = [len(q) for q, _ in reads]
    first = np.concatenate(([0], np.cumsum(Q))).astype(np.uint64)
    return LongCase(np.concatenate([q for q, _ in reads]), first, Q, ref, np.concatenate([p[0] for p in paths]), np.concatenate([p[1] for p in paths]))


@functools.lru_cache(maxsize=None)
def planted_paths():
    """the paths of the restatement of extend: band_ref(q, ref, anchor, 64, 128) per read"""
    ref, sides = planted()
    out = []
    for reads in sides:
        ps = []
        for q, anchor in reads:
            w = band_ref(q, ref, anchor, 64, 128)
            assert w["row"][6] == 0
            ps.append((np.asarray(w["lo"], np.int32), np.asarray(w["hi"], np.int32)))
        out.append(ps)
    return out


def largest_d(rows, k=5, least=8):
    """the k columns of largest D = ks_num / (n_a n_b) among those with n_a, n_b >= least: exact fractions, ties to the smaller column"""
    at = [j for j in range(len(rows)) if rows["n_a"][j] >= least and rows["n_b"][j] >= least]
    d = {j: Fraction(int(rows["ks_num"][j]), int(rows["n_a"][j]) * int(rows["n_b"][j])) for j in at}
    return sorted(at, key=lambda j: (-d[j], j))[:k], d


def contrast_lines(ref, rows, ca, cb, min_depth=1, q0=Q0, shift=SHIFT):
    """the tool's lines, composed from the rows and the two tables"""
    out = []
    for j in np.flatnonzero((rows["depth_a"] >= min_depth) & (rows["depth_b"] >= min_depth)):
        r = rows[j]
        nn = float(r["n_a"]) * float(r["n_b"])
        out.append(b"%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%d\t%s\t%d\t%d\n" % (
            j, ref[j], r["depth_a"], r["depth_b"], ca["n_events"][j], cb["n_events"][j], b"%.6g" % (float(ca["sum_q"][j]) / float(ca["n_events"][j])),
            b"%.6g" % (float(cb["sum_q"][j]) / float(cb["n_events"][j])), b"%.6g" % (float(r["ks_num"]) / nn), q0 + (int(r["ks_bin"]) << shift),
            b"%.6g" % (1.0 - float(r["ov_num"]) / nn), q0 + (int(r["med_a"]) << shift), q0 + (int(r["med_b"]) << shift)))
    return out
