"""The restatement of extend (docs/codecs.md §4.21): band_ref, §4.21 written in int64 numpy with every tile's full D kept for the walk, the
reads that follow a reference (tracking_read, planted_read) and the shapes the CPU and the GPU tests run them at."""
import numpy as np

from chain_common import NO_COST64, PATH_ROW
from dtw_ref import quant_ref

FAR = 1 << 30
QLENS = [1, 63, 64, 65, 127, 128, 129, 200, 321]                           # one tile, exact multiples, one row into the next tile
RLENS = [1, 40, 64, 65, 300]                                               # R < band, windows clipped at 0 and at R - 1
SHAPES = [(64, 64), (64, 128), (128, 128)]                                 # (tile_rows, band)
MIXED_Q = QLENS * 4 + [0, 0, 5, 70]


def band_none(status):
    return dict(row=(NO_COST64, 0, 0, -1, -1, -1, status), a=[], lo=None, hi=None, clamped=0)


def band_ref(q, r, anchor, T=256, band=512, status_in=0, walk=True):
    """§4.21 for ONE query: -> dict(row=(cost, qlen, tiles, start, end, a_last, status), a=[a_k], lo, hi, clamped=carried cells the 2^29 rule
    turned into "no cell").  Every tile's D is kept in int64 (D[i + 1, x + 1] is cell (i, x) of the window; row 0 is the carried row, column
    0 "no cell" left of the window); the walk takes the predecessor of least D, ties to the diagonal, then (i - 1, j), then (i, j - 1), and
    asserts that every cell it visits is real and that the cells' costs sum to `cost`."""
    q = np.asarray(q).astype(np.int64)
    r = np.asarray(r).astype(np.int64)
    Q, R = len(q), len(r)
    assert T in (64, 128, 256, 512, 1024) and band % 64 == 0 and 64 <= band <= 4096 and R >= 1
    if status_in != 0:
        return band_none(status_in)
    if Q == 0:
        return band_none(0)
    if not 0 <= anchor < R:
        return band_none(PATH_ROW)
    INF = np.int64(1) << 40
    amax = max(R - band, 0)
    a = min(max(anchor - band // 4, 0), amax)
    K = (Q + T - 1) // T
    tiles, base, clamped = [], 0, 0
    prev = None                                                            # (a, W, bottom row, min) of the tile before
    for k in range(K):
        qk = q[k * T:(k + 1) * T]
        Qk, W = len(qk), min(band, R - a)
        D = np.full((Qk + 1, W + 1), INF, dtype=np.int64)
        if prev is None:
            D[0, :] = 0
        else:
            pa, pW, pB, pmin = prev
            for x in range(W + 1):                                         # column a + x - 1
                jp = a + x - 1 - pa
                if 0 <= jp < pW and pB[jp] < FAR:
                    if pB[jp] - pmin >= (1 << 29):
                        clamped += 1
                    else:
                        D[0, x] = pB[jp] - pmin
        c = np.abs(qk[:, None] - r[None, a:a + W])
        for d in range(Qk + W - 1):
            i = np.arange(max(0, d - W + 1), min(Qk - 1, d) + 1)
            j = d - i
            D[i + 1, j + 1] = c[i, j] + np.minimum(np.minimum(D[i, j], D[i, j + 1]), D[i + 1, j])
        B = D[Qk, 1:]
        m = int(np.argmin(B))
        mn = int(B[m])
        assert mn < FAR and mn <= 65535 * T and int(B[B < FAR].max()) < FAR
        base += mn
        tiles.append((a, W, D, c))
        prev = (a, W, B, mn)
        end = a + m
        if k + 1 < K:
            a = min(max(end - band // 4, a), amax)
            assert a <= end < a + min(band, R - a)                         # the next window holds m_k
    cost = base
    out = dict(row=(cost, Q, K, -1, end, tiles[-1][0], 0), a=[t[0] for t in tiles], lo=None, hi=None, clamped=clamped)
    if not walk:
        return out
    lo, hi = np.full(Q, -1, dtype=np.int64), np.full(Q, -1, dtype=np.int64)
    k, col, total = K - 1, end, 0
    i = len(tiles[k][2]) - 2
    hi[Q - 1] = end
    while True:
        a, W, D, c = tiles[k]
        x = col - a
        assert 0 <= x < W and D[i + 1, x + 1] < FAR                        # a path cell is real
        total += int(c[i, x])
        gi = k * T + i
        if gi == 0:
            lo[0] = col
            break
        dg, up, lf = D[i, x], D[i, x + 1], D[i + 1, x]
        if dg <= up and dg <= lf:
            lo[gi] = col
            col -= 1
            hi[gi - 1] = col
            i -= 1
        elif up <= lf:
            lo[gi] = col
            hi[gi - 1] = col
            i -= 1
        else:
            col -= 1
        if i < 0:
            k -= 1
            i = len(tiles[k][2]) - 2
    assert total == cost and (lo <= hi).all() and (lo >= 0).all() and set((lo[1:] - hi[:-1]).tolist()) <= {0, 1}
    assert sum(int(np.abs(q[i] - r[lo[i]:hi[i] + 1]).sum()) for i in range(Q)) == cost
    out["row"] = (cost, Q, K, int(lo[0]), end, tiles[-1][0], 0)
    out["lo"], out["hi"] = lo.astype(np.int32), hi.astype(np.int32)
    return out


def tracking_read(rng, Q, R, noise=2.0):
    """a reference of R levels, a query of Q rows that follows it from a random column (each level held 1 or 2 times, the last one to the
    end), and an anchor a few columns off the start"""
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    s = int(rng.integers(0, R))
    cols = np.minimum(s + np.cumsum(rng.integers(0, 2, Q)), R - 1)
    q = np.clip(np.rint(ref[cols] + rng.normal(0.0, noise, Q)), -127, 127).astype(np.int16)
    anchor = int(np.clip(s + rng.integers(-5, 6), 0, R - 1))
    return q, ref, anchor


def planted_read(seed, n_events=3000, R=4096):
    """§4.21's planted case: 4096 levels; a read that walks them from a random column with 5 % of the levels skipped and 1 or 2 events a
    level otherwise (1.5 on average); the event means are the levels through the level change 1.7 x + 30 with a little noise, and the query is
    §4.16's quant of them, as in the chain; the anchor is 7 columns off.  -> (q, ref, anchor, truth): truth[i] is the column of event i"""
    rng = np.random.default_rng(seed)
    ref = np.clip(np.rint(rng.normal(0.0, 40.0, R)), -127, 127).astype(np.int16)
    s = int(rng.integers(64, R - 2200 - 64))
    truth, col = [], s
    while len(truth) < n_events:
        if rng.random() >= 0.05:
            truth += [col] * int(rng.integers(1, 3))
        col += 1
    truth = np.array(truth[:n_events])
    q = quant_ref(1.7 * ref[truth] + 30.0 + rng.normal(0.0, 1.5, n_events))
    return q, ref, s + (7 if seed % 2 else -7), truth


def planted_share(w, truth):
    """the share of events whose span [lo, hi] comes within 2 columns of the truth, and the worst distance"""
    d = np.maximum(np.maximum(w["lo"] - truth, truth - w["hi"]), 0)
    return float((d <= 2).mean()), int(d.max())


def bparams(skip=0, emin=1, emax=1 << 20, tile_rows=256, band=512, clip=127, scale=32.0):
    from slow5tools_amd import _lib

    return _lib.BandParams(skip, emin, emax, tile_rows, band, clip, scale)
