"""Every launch route of the two SIGNAL ENCODERS (csrc/svb_dev.h: svb_tile_classify / svb_tile_write; csrc/exzd_dev.h: exzd_encode_wg; the payload
builders and blob kernels of csrc/encode_kernels.hip) on signals made from the bytes they must produce.

tests/signal_craft.py holds the builders: svb_blob / exzd_blob write a blob field by field, svb_signal / exzd_signal compute the int16 samples
that must encode to given fields.  An entry of the two corpora below is (name, signal, expected blob): the test states codes, positions,
values and q, the signal follows from them, and the expected bytes never pass through an encoder.  (A few entries state their SAMPLES
instead — the guards, the reads around the packed path's range, the reads whose q hangs on one sample: their fields are read off the samples
by svb_fields / fields, the plain numpy statement of the format.)  The CPU tests assert every promise of the corpora from the fields, and
that the oracle encodes every signal to the expected blob and the references decode it back.  They say nothing about the kernels.

The GPU tests send every entry through

  route            call                                                     kernels
  blob-lds         svbzd_encode(), budget 64 KiB                            k_svbzd_encode, assembled in LDS
  blob-hbm         svbzd_encode(), budget 16 bytes                          k_svbzd_encode, byte-wise to HBM from the start
  blob-hbm-late    svbzd_encode(), budget 16384                             ... and from a later tile, after tiles written to LDS
  blob-stream      svbzd_encode_stream()                                    k_svbzd_stream: early groups, groups with a long read, a last
                                                                            group of 1, 2, 3; with a small budget the groups that fail
  none             encode(), REC_NONE                                       k_pack mode 1 (build_payload_hbm)
  fused            encode(), zlib, budget 8192 | 16384                      k_encode_fused<uint32_t | uint64_t, EXZD>, the rest on the list
  tier2            encode(), budget 2048, option fused_tier2 = 16384        two fused launches
  overflow         encode(), budget 48                                      every read on the list: k_pack mode 2 + k_deflate_staged
  all-staged       encode() of a batch with a long read, no budget          k_pack mode 0 + k_deflate_staged
  parked           pack_parked() + deflate_parked()                         the same as two calls
  stream           encode_stream(), budget 16384                            k_encode_stream<uint64_t, EXZD>
  zstd             encode(), REC_ZSTD, budget 16384 | 48                    k_zstd_fused<EXZD> | k_pack + k_zstd_staged

with both signal methods for the record routes, and hold every blob and payload to the expected bytes (a zlib record: what stock zlib
inflates it to; a zstd record: what libzstd makes of it).  Which reads took which route is asserted from what the library shows — the
overflow list, ctl[0] of the single-pass kernels, out_len — against the rules of csrc/enc_plan.h restated here.

Left out: four-byte gaps and values of ex-zd need a read of 2^24 samples (a gap) or cannot come out of int16 samples at all (z <= 131070).
"""
import contextlib
import struct
import zlib

import numpy as np
import pytest

import oracle_bind as ob
import signal_craft as sc

REC_NONE, REC_ZLIB, REC_ZSTD = 0, 1, 2
SVB, EXZD = 1, 2
TILE = 4096                                    # samples (svb-zd) / positions (ex-zd) per tile: 256 lanes of 16
HDR_FIELDS = (8192.0, 23.0, 1467.61, 4000.0)


class Entry:
    def __init__(self, name, x, blob, **f):
        self.name, self.x, self.blob, self.f = name, np.asarray(x, dtype=np.int16), bytes(blob), f


# ---------------------------------------------------------------- the rules of csrc/enc_plan.h, restated
BLK, NARROW, BLOB_MAX = 16384, 8192, 64 * 1024
SIG_RULE = {SVB: (325, 155, 128), EXZD: (950, 130, 256)}      # hundredths of a byte per sample: bound, kept; + bytes of head


def round16(x):
    return (x + 15) & ~15


def fused_cap(sm, max_payload, lds_payload_cap):
    bound, keep, head = SIG_RULE[sm]
    cap = lds_payload_cap if lds_payload_cap else max_payload * keep // bound + head
    return round16(min(cap, max_payload, BLK))


def svb_blob_cap(max_payload, lds_payload_cap, group):
    cap = lds_payload_cap if lds_payload_cap else max_payload * 155 // 325 + 128
    return round16(min(cap * group, BLOB_MAX))


def all_staged(sm, max_payload, lds_payload_cap):
    return not lds_payload_cap and max_payload * 100 // SIG_RULE[sm][0] > 4 * BLK


# ---------------------------------------------------------------- svb-zd corpus
SVB_SIZES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
ALONE_N = 4105                                 # 256 full lanes and one of nine samples
ALONE_AT = (1, 15, 16, 17, 1023, 1024, 4095, 4096, 4097, ALONE_N - 1)
KEYS81 = [(k % 3, k // 3 % 3, k // 9 % 3, k // 27) for k in range(81)]      # the key bytes of int16 input: four codes of 0 .. 2
Z_EDGES = {0: 65535, 1: 131070, 2: 65535, 3: 65536, 4: 255, 5: 256}          # x: -32768, 32767, -1, 32767, 32639, 32767
PACKED_N = 5120                                # five waves of 1024 samples
PACKED_BUT = (("packed_but_sample_1500", 1500, 20000), ("packed_but_sample_2046", 2046, 16384), ("packed_but_sample_2047", 2047, -16385),
              ("packed_but_sample_0", 0, -32768), ("packed_but_sample_5119", 5119, 32767))


def _codes(rng, n):
    c = rng.choice(3, n, p=[0.6, 0.3, 0.1])
    if n and c[0] == 2:
        c[0] = 1
    return c


def _svb(name, codes, rng, **kw):
    x, z = sc.svb_signal(codes, rng, **kw)
    return Entry(name, x, sc.svb_blob(codes, z), codes=np.asarray(codes, dtype=np.int64), z=z)


def _svb_stated(name, x):
    codes, z = sc.svb_fields(x)
    return Entry(name, x, sc.svb_blob(codes, z), codes=codes.astype(np.int64), z=z)


def _svb_corpus():
    rng = np.random.default_rng(0x5B2E)
    out = [_svb("n%d" % n, _codes(rng, n), rng) for n in SVB_SIZES]
    for s in range(4):                                           # lane 0 is filler (a read cannot start with code 2), lane 1 + k holds key byte k in slot s
        codes = _codes(rng, 82 * 16)
        for k, four in enumerate(KEYS81):
            codes[16 * (k + 1) + 4 * s:16 * (k + 1) + 4 * s + 4] = four
        out.append(_svb("keys_slot%d" % s, codes, rng))
    for c in (1, 2):
        for p in ALONE_AT:
            codes = np.zeros(ALONE_N, dtype=np.int64)
            codes[p] = c
            out.append(_svb("code%d_alone_at_%d" % (c, p), codes, rng))
    out.append(_svb("all_code1", np.ones(5000, dtype=np.int64), rng))
    codes = np.full(5000, 2)
    codes[0] = 1
    out.append(_svb("all_code2_behind_the_first", codes, rng))
    codes = _codes(rng, 64)
    codes[:7] = (1, 2, 1, 2, 0, 1, 0)
    out.append(_svb("z_edges", codes, rng, z_at=Z_EDGES))
    # one-byte values for a whole tile, then three-byte ones: 4 + 2049 + 8193 bytes fit a budget of 16384, tile 2's 12288 data bytes do not
    codes = np.zeros(2 * TILE + 1, dtype=np.int64)
    codes[TILE:2 * TILE] = 2
    out.append(_svb("tile2_three_bytes", codes, rng))
    packed, _ = sc.svb_signal((rng.random(PACKED_N) < 0.2).astype(np.int64), rng, lo=-16384, hi=16383)
    out.append(_svb_stated("packed_whole", packed))
    for name, p, v in PACKED_BUT:
        t = packed.copy()
        t[p] = v
        out.append(_svb_stated(name, t))
    return out


def _guard_signals(k):
    """short reads that end in +-32767: the first delta of the read behind one must come from 0, not from its neighbour"""
    rng = np.random.default_rng(0x6A5F + k)
    out = []
    for i in range(k):
        x, _ = sc.svb_signal((rng.random(int(rng.integers(40, 300))) < 0.05).astype(np.int64), rng, lo=-2000, hi=2000)
        out.append(np.concatenate([x, [32767 if i % 2 else -32767]]).astype(np.int16))
    return out


# ---------------------------------------------------------------- ex-zd corpus
EX_SIZES = (0, 1, 2, 3, 17, 18, 4096, 4097, 4098, 8194)
NEX_SMALL = (0, 1, 2, 3, 4, 5)
NEX_TILE = (4095, 4096, 4097)
GAP_EDGES = (255, 256, 65535, 65536)
VAL_EDGES = (0, 255, 256, 65535, 65536, 130814)
Q_BY_SAMPLE_N = 600


def _ex(name, N, q, y0, pos, vals, rng, free=True, force=None):
    """free: the low bit of every val (the sign of its delta) is set against the running sum, as _balance does"""
    pos = np.asarray(pos, dtype=np.int64)
    vals = sc._balance(vals, run=y0) if free else np.asarray(vals, dtype=np.uint64)
    rest = sc.exzd_rest(N, q, y0, pos, vals, rng, force=force)
    x = sc.exzd_signal(N, q, y0, pos, vals, rest)
    return Entry(name, x, sc.exzd_blob(N, q, sc.exzd_z0(y0), sc._gaps(pos), vals, rest), N=N, q=q, y0=y0, pos=pos, vals=np.asarray(vals, dtype=np.int64), rest=rest)


def _ex_walk(name, q, y):
    """the walk stated sample by sample (no step of it may be an exception)"""
    y = np.asarray(y, dtype=np.int64)
    z = sc.zigzag(np.diff(y))
    assert z.max() <= 255
    rest = z.astype(np.uint8).tobytes()
    x = sc.exzd_signal(len(y), q, int(y[0]), [], [], rest)
    return Entry(name, x, sc.exzd_blob(len(y), q, sc.exzd_z0(int(y[0])), [], [], rest), N=len(y), q=q, y0=int(y[0]), pos=np.zeros(0, np.int64),
                 vals=np.zeros(0, np.int64), rest=rest)


def _pick(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), k, replace=False))


def _small_vals(rng, k, top=1200):
    return rng.integers(0, top, k).astype(np.uint64)


def q_range(q):
    return -(32768 >> q), 32767 >> q


def _exzd_corpus():
    rng = np.random.default_rng(0xE72E)
    out = [Entry("N0", np.zeros(0, np.int16), sc.exzd_blob(0, 0, 0, [], [], b""), N=0, q=0, y0=0, pos=np.zeros(0, np.int64), vals=np.zeros(0, np.int64), rest=b"")]
    for N in EX_SIZES[1:]:
        k = min(3, N - 1)
        out.append(_ex("N%d" % N, N, 0, 77, _pick(rng, 0, N - 1, k) if k else [], _small_vals(rng, k), rng))
    # every q: the walk goes from the lowest y that q leaves to the highest in one step, the largest z there is (an exception up to q = 8, a
    # byte of rest from q = 9 on, where the walk is stated sample by sample); the lowest y is negative, the highest is odd
    for q in range(16):
        lo, hi = q_range(q)
        if q <= 8:
            vmax = 2 * (hi - lo) - 256
            pos = [200, 800, 1800, 2600, 3400]
            vals = _small_vals(rng, 5, min(400, vmax - 1))                # (with the low bit set still below vmax)
            vals = sc._balance(vals)
            vals[2] = vmax
            out.append(_ex("q%d_largest_z" % q, 4000, q, 0, pos, vals, rng, free=False))
        else:
            y = rng.integers(lo, hi + 1, 1000)
            y[100], y[101] = lo, hi
            out.append(_ex_walk("q%d_largest_z" % q, q, y))
    for k in (0, 255, 256, Q_BY_SAMPLE_N - 1):                    # every sample a multiple of 16 but one, which is 8 more
        y = 2 * (100 + rng.integers(-15, 16, Q_BY_SAMPLE_N))
        y[k] += 1
        out.append(_ex_walk("q3_by_sample_%d" % k, 3, y))
    out.append(_ex_walk("all_zero", 0, np.zeros(1000, dtype=np.int64)))
    for k in NEX_SMALL:
        out.append(_ex("nex%d" % k, 3000, 0, 300, _pick(rng, 0, 2999, k), _small_vals(rng, k), rng))
    for k in NEX_TILE:                                            # positions 0 .. k - 1: (all but one of / all of / one more than) the first tile
        out.append(_ex("nex%d_dense" % k, 4400, 0, 300, np.arange(k), _small_vals(rng, k), rng))
        out.append(_ex("nex%d_spread" % k, 5 * TILE, 0, 300, _pick(rng, 0, 5 * TILE - 1, k), _small_vals(rng, k), rng))
    out.append(_ex("pos_edges", 9000, 0, 300, [0, 15, 16, 700, 701, 4095, 4096, 8998], _small_vals(rng, 8), rng))
    pos = np.concatenate([_pick(rng, 0, TILE, 6), _pick(rng, 3 * TILE, 4 * TILE, 6)])
    out.append(_ex("tiles_0_and_3", 4 * TILE + 100, 0, 300, pos, _small_vals(rng, 12), rng))
    out.append(_ex("first_exception_at_5000", 9000, 0, 300, [5000, 5001, 8000], _small_vals(rng, 3), rng))
    for g in GAP_EDGES:
        out.append(_ex("gap%d_first" % g, g + 40, 0, 300, [g, g + 7], _small_vals(rng, 2), rng))
    for g in GAP_EDGES[:2]:
        out.append(_ex("gap%d_later" % g, g + 60, 0, 300, [3, 3 + g + 1, 3 + g + 1 + 9], _small_vals(rng, 3), rng))
    out.append(_ex("gap65535_gap65536_later", 131150, 0, 300, [5, 5 + 65536, 5 + 65536 + 65537, 131100], _small_vals(rng, 4), rng))
    # the value widths at their edges: deltas +128, -256, +256, -32896, +32896, +65535 (from -32768 to 32767), and z = 255 (-128) as a byte of rest
    out.append(_ex("val_edges", 6000, 0, 101, [10, 20, 30, 1500, 3000, 5000], VAL_EDGES, rng, free=False, force={5500: 255}))
    # five exceptions, k of their gaps two bytes wide: the position section is 7 + k bytes and the value keys start at byte 31 + k of the blob
    for k in range(4):
        g = np.array([10, 11, 12, 13, 14])
        g[1:1 + k] = 300
        out.append(_ex("vkeys_at_%d" % (31 + k), 1500, 0, 300, np.cumsum(g + 1) - 1, _small_vals(rng, 5), rng))
    return out


SVB_CORPUS = _svb_corpus()
EXZD_CORPUS = _exzd_corpus()
CORPUS = {SVB: SVB_CORPUS, EXZD: EXZD_CORPUS}
GUARDS = _guard_signals(max(len(SVB_CORPUS), len(EXZD_CORPUS)) + 1)
AUX_LENS = (0, 1, 5, 40)
VKEYS = tuple("vkeys_at_%d" % (31 + k) for k in range(4))


class Rec:
    """a read of a batch: signal, expected blob, record head and aux bytes, expected payload"""

    def __init__(self, name, x, blob, i, id_len, aux_len, rng):
        self.name, self.x, self.blob = name, x, blob
        rid = bytes(0x41 + (i + k) % 26 for k in range(id_len))
        self.hdr = struct.pack("<H", id_len) + rid + struct.pack("<Idddd", i, *HDR_FIELDS)
        self.aux = bytes(rng.integers(1, 256, aux_len, dtype=np.uint8))
        self.payload = self.hdr + struct.pack("<Q", len(blob)) + blob + self.aux


def _guard_blob(sm, x):
    return sc.svb_blob(*sc.svb_fields(x)) if sm == SVB else sc.exzd_blob(*sc.fields(x))


_BATCH = {}


def batch(sm):
    """[Rec]: guard, entry, guard, entry, ..., guard; read ids of 1 .. 8 bytes and aux of 0, 1, 5, 40 bytes in every combination; for ex-zd
    the four vkeys entries once more behind it with ids of 1 .. 4 bytes each (the blob starts on every residue of 4)"""
    if sm not in _BATCH:
        rng = np.random.default_rng(0xA11 + sm)
        ents = CORPUS[sm]
        g = GUARDS[:len(ents) + 1]
        items = sc._interleave([(e.name, e.x, e.blob) for e in ents], [("guard", x, _guard_blob(sm, x)) for x in g])
        recs = [Rec(n, x, b, i, 1 + i % 8, AUX_LENS[i // 8 % 4], rng) for i, (n, x, b) in enumerate(items)]
        if sm == EXZD:
            for e in ents:
                if e.name in VKEYS:
                    recs += [Rec(e.name, e.x, e.blob, len(recs), idl, 0, rng) for idl in (1, 2, 3, 4)]
        _BATCH[sm] = recs
    return _BATCH[sm]


# ---------------------------------------------------------------- CPU: the corpora keep their promises
def _by_name(sm):
    d = {e.name: e for e in CORPUS[sm]}
    assert len(d) == len(CORPUS[sm])
    return d


def test_corpus_has_every_promised_shape():
    # ---- svb-zd
    S = _by_name(SVB)
    for e in SVB_CORPUS:                                          # the fields are the signal's: codes at minimal width, z of the deltas from 0
        codes, z = sc.svb_fields(e.x)
        assert np.array_equal(codes, e.f["codes"]) and np.array_equal(z, e.f["z"]) and codes.max(initial=0) <= 2, e.name
    assert [len(S["n%d" % n].x) for n in SVB_SIZES] == list(SVB_SIZES) == [0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
    assert set(S["n8193"].f["codes"].tolist()) == {0, 1, 2}
    for s in range(4):
        c = S["keys_slot%d" % s].f["codes"].reshape(-1, 16)
        assert len(KEYS81) == len(set(KEYS81)) == 81 and [tuple(row[4 * s:4 * s + 4]) for row in c[1:]] == KEYS81
        keys = np.frombuffer(S["keys_slot%d" % s].blob[4:4 + 82 * 4], dtype=np.uint8).reshape(-1, 4)
        assert sorted(keys[1:, s].tolist()) == sorted(a | b << 2 | c_ << 4 | d << 6 for a, b, c_, d in KEYS81)
    assert ALONE_AT == (1, 15, 16, 17, 1023, 1024, 4095, 4096, 4097, 4104) and ALONE_N % 16 == 9
    for c in (1, 2):
        for p in ALONE_AT:
            codes = S["code%d_alone_at_%d" % (c, p)].f["codes"]
            assert len(codes) == ALONE_N and codes[p] == c and codes.sum() == c
    assert (S["all_code1"].f["codes"] == 1).all() and len(S["all_code1"].x) == 5000
    c2 = S["all_code2_behind_the_first"].f["codes"]
    assert c2[0] == 1 and (c2[1:] == 2).all() and len(c2) == 5000
    assert [int(S["z_edges"].f["z"][i]) for i in range(6)] == [65535, 131070, 65535, 65536, 255, 256]
    assert S["z_edges"].x[:2].tolist() == [-32768, 32767]
    t2 = S["tile2_three_bytes"]
    assert (t2.f["codes"][:TILE] == 0).all() and (t2.f["codes"][TILE:2 * TILE] == 2).all() and len(t2.x) == 8193
    assert 4 + 2049 + 8193 <= 16384 < 4 + 2049 + TILE + 3 * TILE        # starts in LDS under a budget of 16384, leaves it in tile 2
    pw = S["packed_whole"].x
    assert len(pw) == PACKED_N and pw.min() >= -16384 and pw.max() < 16384 and set(S["packed_whole"].f["codes"].tolist()) == {0, 1}
    for name, p, v in PACKED_BUT:
        x = S[name].x
        out = np.flatnonzero((x < -16384) | (x >= 16384))
        assert out.tolist() == [p] and x[p] == v, name
    # sample 1500 is seen by wave 1 alone; 2046 and 2047 are the two samples in front of wave 2's first lane: waves 1 and 2 leave the packed path
    assert 1500 // 1024 == 1 and (1500 % 16) not in (14, 15) and 2047 // 1024 == 1 and 2048 % 1024 == 0
    for x in GUARDS:
        assert abs(int(x[-1])) == 32767 and 40 < len(x) <= 300
    assert {int(x[-1]) for x in GUARDS[:4]} == {32767, -32767}
    # ---- ex-zd
    X = _by_name(EXZD)
    for e in EXZD_CORPUS:                                         # the fields are the signal's, q the canonical one
        N, q, z0, gaps, vals, rest = sc.fields(e.x)
        f = e.f
        assert (N, q, z0) == (f["N"], f["q"], sc.exzd_z0(f["y0"]) if N else 0) and rest == f["rest"], e.name
        assert np.array_equal(gaps, sc._gaps(f["pos"])) and np.array_equal(vals, f["vals"]), e.name
    assert [X["N%d" % n].f["N"] for n in EX_SIZES] == [0, 1, 2, 3, 17, 18, 4096, 4097, 4098, 8194]
    for q in range(16):
        e = X["q%d_largest_z" % q]
        lo, hi = q_range(q)
        y = e.x.astype(np.int64) >> q
        zmax = 2 * (hi - lo)
        assert e.f["q"] == q and e.blob[9] == q and y.min() == lo < 0 and y.max() == hi and (e.x < 0).any(), q
        assert int(sc.zigzag(np.diff(y)).max()) == zmax == (1 << (17 - q)) - 2, q
        assert (zmax - 256 in e.f["vals"].tolist()) == (q <= 8) and (q <= 8 or zmax in e.f["rest"]), q
    assert X["q0_largest_z"].f["vals"].max() == 130814
    for k in (0, 255, 256, Q_BY_SAMPLE_N - 1):
        x = X["q3_by_sample_%d" % k].x.astype(np.int64)
        assert len(x) == Q_BY_SAMPLE_N and np.flatnonzero(x & 15).tolist() == [k] and x[k] & 15 == 8
    assert Q_BY_SAMPLE_N % 256 not in (0, 255)                    # the last sample sits in a partly filled stride of 256
    assert not X["all_zero"].x.any() and X["all_zero"].blob[9] == 0 and len(X["all_zero"].x) == 1000
    for k in NEX_SMALL:
        assert len(X["nex%d" % k].f["pos"]) == k == struct.unpack_from("<I", X["nex%d" % k].blob, 12)[0]
    for k in NEX_TILE:
        assert X["nex%d_dense" % k].f["pos"].tolist() == list(range(k))
        p = X["nex%d_spread" % k].f["pos"]
        assert len(p) == k and {int(t) for t in p // TILE} == {0, 1, 2, 3, 4}
    assert NEX_TILE == (TILE - 1, TILE, TILE + 1)
    assert X["pos_edges"].f["pos"].tolist() == [0, 15, 16, 700, 701, 4095, 4096, 9000 - 2]
    assert {int(t) for t in X["tiles_0_and_3"].f["pos"] // TILE} == {0, 3} and X["tiles_0_and_3"].f["N"] > 4 * TILE
    assert X["first_exception_at_5000"].f["pos"][0] == 5000 > TILE
    for g in GAP_EDGES:
        assert sc._gaps(X["gap%d_first" % g].f["pos"])[0] == g
    assert sc._gaps(X["gap255_later"].f["pos"])[1] == 255 and sc._gaps(X["gap256_later"].f["pos"])[1] == 256
    wide = X["gap65535_gap65536_later"]
    assert sc._gaps(wide.f["pos"])[1:3].tolist() == [65535, 65536] and wide.f["N"] == max(e.f["N"] for e in EXZD_CORPUS) == 131150
    assert [int(v) for v in sc._min_codes(GAP_EDGES)] == [0, 1, 1, 2] and [int(v) for v in sc._min_codes(VAL_EDGES)] == [0, 0, 1, 1, 2, 2]
    ve = X["val_edges"]
    assert ve.f["vals"].tolist() == list(VAL_EDGES) and ve.f["q"] == 0
    plain = np.ones(ve.f["N"] - 1, dtype=bool)
    plain[ve.f["pos"]] = False
    assert ve.f["rest"][int(plain[:5500].sum())] == 255 and plain[5500]
    for k, name in enumerate(VKEYS):
        f = X[name].f
        psec, = struct.unpack_from("<I", X[name].blob, 16)
        assert len(f["pos"]) == 5 and psec == 7 + k and 20 + psec + 4 == 31 + k
    assert {(31 + k) % 4 for k in range(4)} == {0, 1, 2, 3}
    # ---- batches: every combination of id and aux length; the vkeys entries with their blob on every residue
    for sm in (SVB, EXZD):
        recs = batch(sm)
        assert {(len(r.hdr) - 38, len(r.aux)) for r in recs} >= {(i, a) for i in range(1, 9) for a in AUX_LENS}
        assert [r.name for r in recs[:2 * len(CORPUS[sm]) + 1:2]] == ["guard"] * (len(CORPUS[sm]) + 1)
        assert all(0 not in r.aux for r in recs)
    for name in VKEYS:
        assert {(len(r.hdr) + 8) % 4 for r in batch(EXZD) if r.name == name} == {0, 1, 2, 3}
    assert sum(len(e.x) for e in SVB_CORPUS) + sum(len(e.x) for e in EXZD_CORPUS) < 700000


@pytest.mark.parametrize("sm", [SVB, EXZD])
def test_builder_equals_the_oracle(sm):
    enc, dec = (ob.svbzd_encode, sc.svb_ref_decode) if sm == SVB else (ob.exzd_encode, sc.exzd_ref_decode)
    for r in batch(sm):
        assert r.blob == enc(r.x), r.name
        assert np.array_equal(dec(r.blob), r.x), r.name
    rec, keep = ob.make_rec(batch(sm)[3].hdr[2:2 + batch(sm)[3].hdr[0]], 3, *HDR_FIELDS, batch(sm)[3].x, batch(sm)[3].aux)
    assert ob.rec_pack(rec, sm) == batch(sm)[3].payload                # and the payload around a blob is the oracle's


# ---------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


@contextlib.contextmanager
def fused_tier2(value):
    from slow5tools_amd import _lib
    L = _lib.lib()
    try:
        _lib.check(L.s5gpu_set_option(b"fused_tier2", value), "s5gpu_set_option")
        yield
    finally:
        _lib.check(L.s5gpu_set_option(b"fused_tier2", 0), "s5gpu_set_option")


def _device_batch(press, recs, sm, rec_method=REC_ZLIB, cap=0, stream=False):
    b = press.DeviceBatch([len(r.x) for r in recs], hdr_len=[len(r.hdr) for r in recs], aux_len=[len(r.aux) for r in recs], rec_method=rec_method,
                          sig_method=sm, lds_payload_cap=cap, with_stream_out=stream)
    b.upload([r.x for r in recs], [r.hdr for r in recs], [r.aux for r in recs])
    return b


def _same(where, got, want):
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes for %d, first difference at byte %d" % (where, len(got), len(want), k))


def _check_records(route, recs, out, rec_method):
    assert len(out) == len(recs)
    for i, (r, rec) in enumerate(zip(recs, out)):
        where = (route, i, r.name)
        assert len(rec) >= 8 and struct.unpack_from("<Q", rec, 0)[0] == len(rec) - 8, where
        body = rec[8:]
        if rec_method == REC_NONE:
            got = body
        elif rec_method == REC_ZLIB:
            assert body[:2] == b"\x78\x9c", where
            got = zlib.decompress(body)
        else:
            got = ob.zstd_decompress(body, len(r.payload))
            assert got is not None, where
        _same(where, got, r.payload)


def _listed(b):
    b.torch.cuda.synchronize(b.dev)
    ovf = b.ovf.cpu().numpy()
    out = set(int(v) for v in ovf[1:1 + int(ovf[0])])
    assert len(out) == int(ovf[0])
    return out


def _fit_rule(recs, cap):
    """(must be declined, must not be): a payload longer than the budget cannot fit; one with 16 bytes to spare must (the encoders' word-wide
    ORs and the budget's rounding to 16 are inside that)"""
    return {i for i, r in enumerate(recs) if len(r.payload) > cap}, {i for i, r in enumerate(recs) if len(r.payload) + 16 <= cap}


def _report(route, sm, recs, **groups):
    """one line per route: how many reads took each way, and how many of them are corpus entries (the others are the guards between them)"""
    parts = []
    for k, idx in groups.items():
        idx = list(idx)
        parts.append("%s %d reads (%d entries)" % (k, len(idx), sum(recs[i].name != "guard" for i in idx)))
    print("%s %s: %s" % (route, "svb-zd" if sm == SVB else "ex-zd", ", ".join(parts)))


# ---- svb-zd blobs alone
def _blob_route(press, recs, cap):
    b = _device_batch(press, recs, SVB, cap=cap)
    b.svbzd_encode()
    for i, (r, blob) in enumerate(zip(recs, b.records())):
        _same(("blob", cap, i, r.name), blob, r.blob)
    pc = svb_blob_cap(b.tot["max_payload"], cap, 1)
    n = [len(r.x) for r in recs]
    up_front = {i for i in range(len(recs)) if 4 + (n[i] + 3) // 4 + n[i] > pc}
    late = {i for i, r in enumerate(recs) if i not in up_front and len(r.blob) > pc}
    return pc, up_front, late


@pytest.mark.gpu
def test_blob_kernel_lds_form(press):
    """k_svbzd_encode with the largest budget: every blob is assembled in LDS"""
    recs = batch(SVB)
    pc, up_front, late = _blob_route(press, recs, BLOB_MAX)
    assert pc == BLOB_MAX and not up_front and not late
    _report("blob-lds", SVB, recs, lds=range(len(recs)))


@pytest.mark.gpu
def test_blob_kernel_hbm_fallback_up_front(press):
    """a budget of 16 bytes: reads of ten samples or more cannot fit at a byte per sample and are written byte-wise to HBM from the start"""
    recs = batch(SVB)
    pc, up_front, late = _blob_route(press, recs, 16)
    assert pc == 16 and {r.name for i, r in enumerate(recs) if i not in up_front} == {"n0", "n1", "n2", "n3", "n4", "n5"}
    _report("blob-hbm", SVB, recs, up_front=up_front, late=late, lds=set(range(len(recs))) - up_front - late)


@pytest.mark.gpu
def test_blob_kernel_hbm_fallback_in_a_later_tile(press):
    """a budget of 16384: tile2_three_bytes (8193 samples) passes the test up front, its first tile of one-byte values is written to LDS,
    the second tile's three-byte values no longer fit — and every other read goes the way the rule says"""
    recs = batch(SVB)
    pc, up_front, late = _blob_route(press, recs, 16384)
    assert pc == 16384 and not up_front and "tile2_three_bytes" in {recs[i].name for i in late}
    t2 = next(r for r in recs if r.name == "tile2_three_bytes")
    assert 4 + 2049 + TILE <= pc < len(t2.blob)
    _report("blob-hbm-late", SVB, recs, late=late, lds=set(range(len(recs))) - late)


def _stream_plan(recs, cap):
    """k_svbzd_stream restated: -> (kind of every group, the reads that fit).  A full group of single-tile reads whose blobs fit together is
    written at once ("early"); otherwise read by read, each behind the ones that fitted"""
    kinds, fits = [], set()
    for g0 in range(0, len(recs), 4):
        idx = range(g0, min(g0 + 4, len(recs)))
        full, single = len(idx) == 4, all(len(recs[i].x) <= TILE for i in idx)
        if full and single and sum(len(recs[i].blob) for i in idx) <= cap:
            kinds.append("early")
            fits |= set(idx)
            continue
        pos = 0
        for i in idx:
            if pos + len(recs[i].blob) <= cap:
                pos += len(recs[i].blob)
                fits.add(i)
        ok = all(i in fits for i in idx)
        kinds.append(("tail%d" % len(idx) if not full else "long" if not single else "refused") + ("" if ok else "_partly"))
    return kinds, fits


def _stream_route(press, recs, cap):
    b = _device_batch(press, recs, SVB, cap=cap, stream=True)
    b.svbzd_encode_stream()
    data, off = b.stream_bytes()
    ctl = b.lb_ctl.cpu().numpy()
    lens = b.out_len[:len(recs)].cpu().numpy()
    kinds, fits = _stream_plan(recs, svb_blob_cap(b.tot["max_payload"], cap, 4))
    assert int(ctl[2]) == 0 and int(ctl[0]) == len(recs) - len(fits) and b.stream_ok() == (len(fits) == len(recs))
    for i, r in enumerate(recs):
        got = data[int(off[i]):int(off[i + 1])]
        _same(("blob-stream", cap, i, r.name), got, r.blob if i in fits else b"")
        assert int(lens[i]) == len(got)
    return kinds, fits


@pytest.mark.gpu
def test_blob_stream_groups_that_fit(press):
    """k_svbzd_stream, 64 KiB for a group: groups of four single-tile reads (the early form), groups with a read of more than 4096
    samples, and — the batch cut to 5, 6 and 7 reads — a last group of 1, 2 and 3"""
    recs = batch(SVB)
    kinds, fits = _stream_route(press, recs, 16384)
    assert len(fits) == len(recs) and kinds.count("early") >= 8 and kinds.count("long") >= 5 and set(kinds) <= {"early", "long", "tail1", "tail2", "tail3"}
    at = next(i for i, r in enumerate(recs) if r.name == "n4097") // 4 * 4       # a full group with a long read, then 1, 2, 3 more
    for k in (1, 2, 3):
        kk, ff = _stream_route(press, recs[at:at + 4 + k], 16384)
        assert kk == ["long", "tail%d" % k] and len(ff) == 4 + k
    _report("blob-stream", SVB, recs, **{k: [i for i in range(len(recs)) if kinds[i // 4] == k] for k in sorted(set(kinds))})


@pytest.mark.gpu
def test_blob_stream_groups_that_do_not_fit(press):
    """4096 bytes for a group: groups of single-tile reads fail `need <= cap` and are redone read by read — the reads that fit come out
    right, the others are reported (length 0, ctl[0] counts them, stream_ok() is false)"""
    recs = batch(SVB)
    kinds, fits = _stream_route(press, recs, 1024)
    assert kinds.count("refused_partly") >= 3 and kinds.count("early") >= 3 and kinds.count("long_partly") >= 5 and 20 <= len(fits) < len(recs)
    # in some refused group a read fits BEHIND one that did not
    assert any(i not in fits and i + 1 in fits and i // 4 == (i + 1) // 4 for i in range(len(recs) - 1))
    _report("blob-stream-refused", SVB, recs, fit=fits, reported=set(range(len(recs))) - fits, **{k: [i for i in range(len(recs)) if kinds[i // 4] == k] for k in sorted(set(kinds))})


# ---- records
SM = pytest.mark.parametrize("sm", [SVB, EXZD])


@SM
@pytest.mark.gpu
def test_route_record_press_none(press, sm):
    """k_pack mode 1: the payload, assembled tile by tile in LDS and copied out (svb-zd) or written in place (ex-zd), is the record"""
    recs = batch(sm)
    b = _device_batch(press, recs, sm, REC_NONE)
    b.encode()
    _check_records("none", recs, b.records(), REC_NONE)
    _report("none", sm, recs, k_pack=range(len(recs)))


@SM
@pytest.mark.parametrize("budget", [NARROW, BLK])
@pytest.mark.gpu
def test_route_fused(press, sm, budget):
    """zlib, one fused launch with a budget of 8192 (the uint32_t kernels) and of 16384 (uint64_t): the payload is built in LDS; what does
    not fit is on the overflow list and redone by k_pack mode 2 + k_deflate_staged"""
    recs = batch(sm)
    with fused_tier2(0):
        b = _device_batch(press, recs, sm, cap=budget)
        b.encode()
        out = b.records()
    cap = fused_cap(sm, b.tot["max_payload"], budget)
    assert cap == budget
    listed, (must, must_not) = _listed(b), _fit_rule(recs, cap)
    assert must <= listed and not (listed & must_not) and len(recs) - len(listed) >= 60
    _check_records("fused %d" % budget, recs, out, REC_ZLIB)
    _report("fused-%d" % budget, sm, recs, fused=set(range(len(recs))) - listed, listed=listed)


@SM
@pytest.mark.gpu
def test_route_second_fused_launch(press, sm):
    """option fused_tier2: a first fused launch with 2048 bytes, a second with one block; only what fits neither is on the list"""
    recs = batch(sm)
    with fused_tier2(BLK):
        b = _device_batch(press, recs, sm, cap=2048)
        b.encode()
        out = b.records()
    listed, (must, must_not) = _listed(b), _fit_rule(recs, BLK)
    first = _fit_rule(recs, 2048)
    assert must <= listed and not (listed & must_not)
    assert len(first[1]) >= 15 and len(must_not - first[1]) >= 20 and len(first[0] & must_not) >= 20       # reads for the first launch, and for the second alone
    _check_records("tier2", recs, out, REC_ZLIB)
    _report("tier2", sm, recs, first_launch=first[1], second_launch=set(range(len(recs))) - listed - first[1], listed=listed)


@SM
@pytest.mark.gpu
def test_route_overflow_list(press, sm):
    """a budget below every payload: the fused launch declines every read, k_pack mode 2 + k_deflate_staged take them from the list"""
    recs = batch(sm)
    with fused_tier2(0):
        b = _device_batch(press, recs, sm, cap=48)
        b.encode()
        out = b.records()
    assert min(len(r.payload) for r in recs) > 48 and _listed(b) == set(range(len(recs)))
    _check_records("overflow", recs, out, REC_ZLIB)
    _report("overflow", sm, recs, listed=range(len(recs)))


LONG_READ = 70000                 # samples of the read that makes a batch "long" (s5plan::all_staged)


@SM
@pytest.mark.gpu
def test_route_all_staged(press, sm):
    """a batch with one long read and no budget named: k_pack mode 0 + k_deflate_staged over every read, nothing on the list"""
    rng = np.random.default_rng(9)
    x = ob.synth_read(0x5105, 0, LONG_READ)
    recs = batch(sm) + [Rec("long", x, ob.svbzd_encode(x) if sm == SVB else ob.exzd_encode(x), 999, 4, 0, rng)]
    b = _device_batch(press, recs, sm)
    assert all_staged(sm, b.tot["max_payload"], 0)
    b.encode()
    out = b.records()
    assert not _listed(b)
    _check_records("all-staged", recs, out, REC_ZLIB)
    _report("all-staged", sm, recs, staged=range(len(recs)))


@SM
@pytest.mark.gpu
def test_route_parked(press, sm):
    """pack_parked() + deflate_parked(): the two steps of the staged path as two calls"""
    recs = batch(sm)
    b = _device_batch(press, recs, sm)
    b.pack_parked()
    b.torch.cuda.synchronize(b.dev)
    assert b.out_len[:len(recs)].cpu().numpy().tolist() == [len(r.payload) for r in recs]       # the parked payloads' lengths
    b.deflate_parked()
    _check_records("parked", recs, b.records(), REC_ZLIB)
    _report("parked", sm, recs, parked=range(len(recs)))


@SM
@pytest.mark.gpu
def test_route_encode_stream(press, sm):
    """encode_stream() with a budget of one block: every read that fits is in the stream, byte for byte the record encode() leaves in its
    slot; the others are reported (size 0, ctl[0]); the reads that certainly fit, alone, make a valid stream"""
    recs = batch(sm)
    must, must_not = _fit_rule(recs, BLK)

    def run(rs):
        b = _device_batch(press, rs, sm, cap=BLK, stream=True)
        b.encode_stream()
        got = b.stream_records(range(len(rs)))
        ctl = b.lb_ctl.cpu().numpy()
        assert fused_cap(sm, b.tot["max_payload"], BLK) == BLK and int(ctl[2]) == 0
        return b, got, int(ctl[0])

    b, got, n_failed = run(recs)
    failed = {i for i, g in enumerate(got) if not g}
    assert n_failed == len(failed) and must <= failed and not (failed & must_not) and not b.stream_ok()
    _check_records("stream", [r for i, r in enumerate(recs) if i not in failed], [g for g in got if g], REC_ZLIB)
    with fused_tier2(0):
        b.encode()
        assert [r for i, r in enumerate(b.records()) if i not in failed] == [g for g in got if g]
    fit = [r for i, r in enumerate(recs) if i in must_not]
    b2, got2, n2 = run(fit)
    assert n2 == 0 and b2.stream_ok()
    _check_records("stream, all fit", fit, got2, REC_ZLIB)
    _report("stream", sm, recs, in_stream=set(range(len(recs))) - failed, reported=failed)


@SM
@pytest.mark.gpu
def test_route_zstd(press, sm):
    """zstd records: k_zstd_fused with a budget of one block (the rest through the list to k_zstd_staged), and every read staged (budget
    48); libzstd recovers the payload"""
    if ob.zstd_ref() is None:
        pytest.skip("no libzstd.so.1 in this image")
    recs = batch(sm)
    b = _device_batch(press, recs, sm, REC_ZSTD, cap=BLK)
    b.encode()
    out = b.records()
    listed, (must, must_not) = _listed(b), _fit_rule(recs, BLK)
    assert must <= listed and not (listed & must_not) and len(recs) - len(listed) >= 60
    _check_records("zstd fused", recs, out, REC_ZSTD)
    b = _device_batch(press, recs, sm, REC_ZSTD, cap=48)
    b.encode()
    out = b.records()
    assert _listed(b) == set(range(len(recs)))
    _check_records("zstd staged", recs, out, REC_ZSTD)
    _report("zstd", sm, recs, fused=set(range(len(recs))) - listed, listed=listed, all_staged_run=range(len(recs)))


EDGE_ENTRY = {SVB: "n1025", EXZD: "nex5"}


@SM
@pytest.mark.gpu
def test_the_budget_edge_byte_by_byte(press, sm):
    """one signal with aux of 0 .. 32 bytes under a budget of the shortest payload + 16: the payloads run in one-byte steps from 16 below
    the budget to 16 above it.  Every record is right; every read whose payload exceeds the budget is on the overflow list; none with
    payload + 16 <= budget is; both happen"""
    e = _by_name(sm)[EDGE_ENTRY[sm]]
    rng = np.random.default_rng(77)
    id_len = (-(38 + 8 + len(e.blob))) % 16 or 16
    recs = [Rec(e.name, e.x, e.blob, k, id_len, k, rng) for k in range(33)]
    budget = len(recs[0].payload) + 16
    assert budget % 16 == 0 and [len(r.payload) for r in recs] == list(range(budget - 16, budget + 17))
    with fused_tier2(0):
        b = _device_batch(press, recs, sm, cap=budget)
        b.encode()
        out = b.records()
    assert fused_cap(sm, b.tot["max_payload"], budget) == budget
    listed, (must, must_not) = _listed(b), _fit_rule(recs, budget)
    assert must == set(range(17, 33)) and must_not == {0}
    assert must <= listed and not (listed & must_not)
    _check_records("budget edge", recs, out, REC_ZLIB)
    print("budget edge %s: budget %d, payloads on the list: %s" % ("svb-zd" if sm == SVB else "ex-zd", budget, sorted(len(recs[i].payload) for i in listed)))
