"""diff: per-read signal error and field differences between two files, compared on the device (k_sig_diff, docs/codecs.md §4.14), the C
calls, slow5tools_amd.diff and the s5diff tool.

The oracle is pair_ref / acc_ref in this file: the per-pair rule restated in numpy (int64 arithmetic, Python integers for the 64-bit sums that
wrap) over int16 arrays a test made itself or that the oracle's decoders produced (`pieces` / `depress` as in tests/test_digest.py).  Every
member is an integer sum, maximum or count, so every comparison is exact.

  not gpu : exported symbols and bindings, the layout of the two structs against the numpy dtypes, the oracle on a hand-made case and pinned on
            the reference's own degrade pairs.
  gpu     : crafted pairs of every length step of the kernel (lane 8, wave 512, workgroup 2048 samples per step) and content kind; the nine
            press pairs; s5gpu_signal_diff_dev over two device decodes between guard words; corrupt and truncated records on either side; the
            accumulator under every option; the s5diff tool on the reference's files.
"""
import ctypes as C
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import GOLDEN, Blow5, golden
from zstd_craft import xxh64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S5DIFF = os.path.join(ROOT, "slow5tools_amd", "s5diff")
S5VIEW = os.path.join(ROOT, "slow5tools_amd", "s5view")
NAMES = ["s5gpu_diff_acc_bytes", "s5gpu_diff_acc_reset_dev", "s5gpu_signal_diff_dev", "s5gpu_diff_open", "s5gpu_diff_add_batch", "s5gpu_diff_close"]
PRESSES = [(r, s) for r in (ob.REC_NONE, ob.REC_ZLIB, ob.REC_ZSTD) for s in (ob.SIG_NONE, ob.SIG_SVB_ZD, ob.SIG_EX_ZD)]
GUARD = 0xA5A5A5A5A5A5A5A5
NONE = 0xFFFFFFFF
SIGNAL, LEN, READ_GROUP, DIGITISATION, OFFSET, RANGE, SAMPLING_RATE, ID, AUX = (1 << k for k in range(9))
FAILED, BAD_PAIR = 0x4000, 0x8000
FLAG_NAMES = ["signal", "len", "read_group", "digitisation", "offset", "range", "sampling_rate", "id", "aux"]
M64 = 2 ** 64 - 1
DOUBLES = (8192.0, 23.0, 1467.61, 4000.0)


# ---------------------------------------------------------------------------------------------------------------- the oracle

class Read:
    """one side of a pair as the oracle sees it"""

    def __init__(self, rid, rg, doubles, sig, aux=b""):
        self.rid, self.rg, self.aux = bytes(rid), int(rg), bytes(aux)
        self.dbits = [struct.pack("<d", x) for x in doubles]            # compared bit for bit
        self.doubles = tuple(doubles)
        self.sig = np.ascontiguousarray(sig, dtype=np.int16)

    def stored(self, rec_method, sig_method):
        """the record as a BLOW5 file with these presses stores it (without the u64 prefix)"""
        r, keep = ob.make_rec(self.rid, self.rg, *self.doubles, self.sig, self.aux)
        if rec_method == ob.REC_ZSTD:
            pay = ob.rec_pack(r, sig_method)
            return ob.zstd_compress(pay) if ob.zstd_ref() else ob.zstd_literals_compress(pay)
        return ob.rec_to_mem(r, rec_method, sig_method)[8:]


def depress(rec, rec_method):
    if rec_method == ob.REC_ZLIB:
        return zlib.decompress(rec)
    if rec_method == ob.REC_ZSTD:
        out = ob.zstd_decompress(rec) if ob.zstd_ref() else ob.zstd_restated_decompress(rec, 16 * len(rec) + (1 << 20))
        assert out is not None
        return out
    return bytes(rec)


def pieces(payload, sig_method):
    """(head, samples, aux) of an uncompressed record: head = u16 id_len | id | u32 read_group | 4 x f64"""
    (idl,) = struct.unpack_from("<H", payload, 0)
    hl = 2 + idl + 36
    (L,) = struct.unpack_from("<Q", payload, hl)
    if sig_method == ob.SIG_NONE:
        nb = 2 * L
        sig = np.frombuffer(payload, dtype="<i2", count=L, offset=hl + 8)
    else:
        nb = L
        blob = payload[hl + 8:hl + 8 + L]
        sig = ob.svbzd_decode(blob) if sig_method == ob.SIG_SVB_ZD else ob.exzd_decode(blob)
        assert sig is not None
    return payload[:hl], np.asarray(sig, dtype=np.int16), payload[hl + 8 + nb:]


def read_of(rec, rec_method, sig_method):
    """a stored record through the oracle's decoders"""
    head, sig, aux = pieces(depress(rec, rec_method), sig_method)
    idl = len(head) - 38
    (rg,) = struct.unpack_from("<I", head, 2 + idl)
    return Read(head[2:2 + idl], rg, struct.unpack_from("<4d", head, 6 + idl), sig, aux)


def file_reads(path):
    f = Blow5(path)
    return [read_of(r, f.rec_method, f.sig_method) for r in f.records], f


def diff_of(a, b):
    n = min(a.sig.size, b.sig.size)
    return b.sig[:n].astype(np.int64) - a.sig[:n].astype(np.int64)


def failed_row(status_a, status_b, flags=FAILED):
    from slow5tools_amd._lib import SIG_DIFF

    r = np.zeros(1, dtype=SIG_DIFF)[0]
    r["status_a"], r["status_b"], r["flags"], r["first_diff"], r["max_at"] = status_a, status_b, flags, NONE, NONE
    return r


def pair_ref(a, b, payload=True):
    """the row of s5gpu_sig_diff_t the definition gives for reads a and b"""
    from slow5tools_amd._lib import SIG_DIFF

    r = np.zeros(1, dtype=SIG_DIFF)[0]
    d = diff_of(a, b)
    n = d.size
    x = a.sig[:n].astype(np.int64)
    nz = np.nonzero(d)[0]
    ad = np.abs(d)
    fl = (SIGNAL if nz.size else 0) | (LEN if a.sig.size != b.sig.size else 0) | (READ_GROUP if a.rg != b.rg else 0)
    for k, bit in enumerate((DIGITISATION, OFFSET, RANGE, SAMPLING_RATE)):
        fl |= bit if a.dbits[k] != b.dbits[k] else 0
    if payload:
        fl |= (ID if a.rid != b.rid else 0) | (AUX if a.aux != b.aux else 0)
    r["n_a"], r["n_b"], r["flags"], r["n_diff"] = a.sig.size, b.sig.size, fl, nz.size
    r["first_diff"] = int(nz[0]) if nz.size else NONE
    r["max_abs"] = int(ad.max()) if n else 0
    r["max_at"] = int(np.argmax(ad)) if nz.size else NONE               # argmax: the first of equal maxima
    r["sum_d"], r["sum_abs"], r["sum_sq"] = int(d.sum()), int(ad.sum()), int((d * d).sum())
    r["sum_a"], r["sumsq_a"] = int(x.sum()), int((x * x).sum())
    return r


def acc_ref(rows, ds):
    """the accumulator of the pairs with rows `rows`; ds: the differences of the pairs that are not failed, in any order"""
    from slow5tools_amd._lib import DIFF_ACC

    o = np.zeros(1, dtype=DIFF_ACC)[0]
    fields = READ_GROUP | DIGITISATION | OFFSET | RANGE | SAMPLING_RATE
    good = [r for r in rows if not r["flags"] & (FAILED | BAD_PAIR)]
    o["n_pairs"], o["n_failed"] = len(rows), len(rows) - len(good)
    o["n_differ"] = sum(1 for r in good if r["flags"])
    for name, bit in (("n_signal", SIGNAL), ("n_len", LEN), ("n_fields", fields), ("n_aux", AUX), ("n_id", ID)):
        o[name] = sum(1 for r in good if r["flags"] & bit)
    o["n_samples"] = sum(min(int(r["n_a"]), int(r["n_b"])) for r in good)
    for name in ("n_diff", "sum_abs", "sum_sq", "sumsq_a"):
        o[name] = sum(int(r[name]) for r in good) & M64
    for name in ("sum_d", "sum_a"):
        v = sum(int(r[name]) for r in good) & M64
        o[name] = v - 2 ** 64 if v >= 2 ** 63 else v
    o["max_abs"] = max([int(r["max_abs"]) for r in good] + [0])
    d = np.concatenate([np.asarray(x, dtype=np.int64) for x in ds] + [np.zeros(0, np.int64)])
    assert d.size == o["n_samples"]
    o["hist"][:] = np.bincount(d + 65535, minlength=131071)
    return o


def assert_same(got, want, what=""):
    for name in want.dtype.names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if not np.array_equal(g, w):
            at = np.nonzero(np.atleast_1d(g != w))[0][:8]
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, at.tolist(), np.atleast_1d(g)[at].tolist(), np.atleast_1d(w)[at].tolist()))


def qts(x, bits):
    """docs/codecs.md §4.8 restated"""
    y = ((x.astype(np.int32) + (1 << (bits - 1))) >> bits) << bits
    return np.where(y > 32767, y - (1 << bits), y).astype(np.int16)


# ---------------------------------------------------------------------------------------------------------------- crafted pairs

# the lane (8 samples), wave (512) and workgroup (2048) steps of the 16-byte loads, and one read that needs many steps
LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4000, 4097, 70001]
STEPS = [8, 16, 64, 512, 2048]


def raw_like(n, rng):
    return np.clip(np.rint(520 + 90 * rng.standard_normal(n)), -400, 1400).astype(np.int16)


def crafted_pairs():
    """[(what, Read a, Read b)] : every length x every content kind; ids and aux equal unless the kind says otherwise"""
    rng = np.random.default_rng(414)
    out = []

    def add(what, a, b, **kw):
        k = len(out)
        rid = b"pair-%05d" % k
        out.append((what, Read(kw.get("ida", rid), kw.get("rga", 1), kw.get("da", DOUBLES), a, kw.get("auxa", b"\x01\x02\x03")),
                    Read(kw.get("idb", rid), kw.get("rgb", 1), kw.get("db", DOUBLES), b, kw.get("auxb", b"\x01\x02\x03"))))

    for n in LENGTHS:
        x = raw_like(n, rng)
        add("identical %d" % n, x, x.copy())
        at = sorted({p for p in [0, n - 1] + [s + e for s in STEPS for e in (-1, 0, 1)] if 0 <= p < n})
        for p in at:
            y = x.copy()
            y[p] += 3
            add("one sample at %d of %d" % (p, n), x, y)
        lo, hi = np.full(n, -32768, np.int16), np.full(n, 32767, np.int16)
        add("d = +65535 everywhere %d" % n, lo, hi)
        add("d = -65535 everywhere %d" % n, hi, lo)
        add("+1 everywhere %d" % n, x, (x + 1).astype(np.int16))
        for bits in (1, 3, 16):
            add("rounded at %d bits %d" % (bits, n), x, qts(x, bits))
        r1, r2 = (rng.integers(-32768, 32768, size=n, dtype=np.int32).astype(np.int16) for _ in range(2))
        add("random %d" % n, r1, r2)
        if n >= 2:
            y = x.copy()
            p, q = sorted(rng.choice(n, size=2, replace=False))
            y[p] -= 77
            y[q] += 77
            add("two positions tie for max_abs %d" % n, x, y)
        wild = rng.integers(-32768, 32768, size=n + 37, dtype=np.int32).astype(np.int16)
        wild[:n] = x
        if n:
            wild[n // 2] ^= 1
        add("b longer %d" % n, x, wild)
        add("a longer %d" % n, wild, x)
    x = raw_like(100, rng)
    add("read_group alone", x, x, rga=1, rgb=2)
    for k, name in enumerate(("digitisation", "offset", "range", "sampling_rate")):
        d2 = list(DOUBLES)
        d2[k] += 0.5
        add(name + " alone", x, x, db=tuple(d2))
    add("0.0 against -0.0", x, x, da=(8192.0, 0.0, 1467.61, 4000.0), db=(8192.0, -0.0, 1467.61, 4000.0))
    add("equal-bit NaNs", x, x, da=(8192.0, float("nan"), 1467.61, 4000.0), db=(8192.0, float("nan"), 1467.61, 4000.0))
    add("aux differs in the last byte", x, x, auxa=bytes(range(40)), auxb=bytes(range(39)) + b"\xff")
    add("aux of different lengths", x, x, auxa=bytes(range(40)), auxb=bytes(range(41)))
    add("aux empty against non-empty", x, x, auxa=b"", auxb=b"\x07")
    add("aux empty on both sides", x, x, auxa=b"", auxb=b"")
    add("aux of 700 bytes differs at byte 300", x, x, auxa=bytes(700), auxb=bytes(300) + b"\x01" + bytes(399))
    add("ids differ in the last byte", x, x, ida=b"read-x", idb=b"read-y")
    add("ids of different lengths", x, x, ida=b"read-x", idb=b"read-xx")
    return out


class Crafted:
    def __init__(self):
        self.pairs = crafted_pairs()
        self.rows = [pair_ref(a, b) for _, a, b in self.pairs]
        self.ds = [diff_of(a, b) for _, a, b in self.pairs]
        self.stored_a = [a.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD) for _, a, _b in self.pairs]
        self.stored_b = [b.stored(ob.REC_ZLIB, ob.SIG_EX_ZD) for _, _a, b in self.pairs]
        self.extreme = [i for i, (w, _a, _b) in enumerate(self.pairs) if w.startswith("d = ") and self.rows[i]["n_a"]]

    def subset(self, idx):
        return [self.rows[i] for i in idx], [self.ds[i] for i in idx]


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


def flags_of(crafted, what):
    (i,) = [k for k, (w, _a, _b) in enumerate(crafted.pairs) if w == what]
    return int(crafted.rows[i]["flags"])


def test_the_crafted_pairs_hold_what_the_kernel_can_get_wrong(crafted):
    """asserted on the CPU, before any GPU test relies on it"""
    rows = crafted.rows
    assert len(rows) > 400 and max(int(r["max_abs"]) for r in rows) == 65535
    assert flags_of(crafted, "identical 4000") == 0 and flags_of(crafted, "+1 everywhere 513") == SIGNAL
    assert flags_of(crafted, "b longer 0") == LEN and flags_of(crafted, "a longer 2049") == SIGNAL | LEN
    assert flags_of(crafted, "read_group alone") == READ_GROUP and flags_of(crafted, "range alone") == RANGE
    assert flags_of(crafted, "0.0 against -0.0") == OFFSET and flags_of(crafted, "equal-bit NaNs") == 0
    assert flags_of(crafted, "aux differs in the last byte") == AUX and flags_of(crafted, "aux of different lengths") == AUX
    assert flags_of(crafted, "aux empty against non-empty") == AUX and flags_of(crafted, "aux empty on both sides") == 0
    assert flags_of(crafted, "ids differ in the last byte") == ID and flags_of(crafted, "ids of different lengths") == ID
    tie = [r for (w, _a, _b), r in zip(crafted.pairs, rows) if w.startswith("two positions tie")]
    assert all(r["max_abs"] == 77 and r["n_diff"] == 2 and r["max_at"] == r["first_diff"] for r in tie)
    sq = [r for (w, _a, _b), r in zip(crafted.pairs, rows) if w == "d = -65535 everywhere 70001"][0]
    assert sq["sum_sq"] == 70001 * 65535 ** 2 and sq["sum_d"] == -70001 * 65535 and sq["sumsq_a"] == 70001 * 32767 ** 2
    want = acc_ref(rows, crafted.ds)
    assert want["hist"][0] > 0 and want["hist"][131070] > 0 and want["hist"][65535] == want["n_samples"] - want["n_diff"]
    # a window of 8 bins holds d = -4 .. 3: rounding at 3 bits gives d = 4 as well, so both the LDS window and the global path run
    assert want["hist"][65535 + 4] > 0 and want["hist"][65535 - 4] > 0 and want["hist"][65535 + 3] > 0


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_and_binds_the_diff_calls():
    from slow5tools_amd import _lib, diff

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in NAMES if s not in exported] and not [s for s in NAMES if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert len(L.s5gpu_signal_diff_dev.argtypes) == 8 and len(L.s5gpu_diff_add_batch.argtypes) == 13 and len(L.s5gpu_diff_close.argtypes) == 2
    assert callable(diff.pair_diffs) and callable(diff.file_diff) and callable(diff.diff_dev)
    assert os.access(S5DIFF, os.X_OK)
    for key, bad in ((b"diff_lds_bins", 4), (b"diff_lds_bins", 100), (b"diff_lds_bins", 512), (b"diff_flush_samples", 0), (b"diff_grid", 0), (b"diff_grid", 1025)):
        assert L.s5gpu_set_option(key, bad) == -1
    for key, good in ((b"diff_lds_bins", 64), (b"diff_flush_samples", 0xFFFFFFFF), (b"diff_grid", 1024)):
        assert L.s5gpu_set_option(key, good) == 0                 # (the defaults)


def test_the_numpy_dtypes_are_the_c_structs(tmp_path):
    from slow5tools_amd import _lib

    src = tmp_path / "d.c"
    text = '#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){\n'
    for st, dt in (("s5gpu_sig_diff_t", _lib.SIG_DIFF), ("s5gpu_diff_acc_t", _lib.DIFF_ACC)):
        text += 'printf("%%zu", sizeof(%s));\n' % st + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (st, n) for n in dt.names) + 'printf("\\n");\n'
    text += 'printf("%zu\\n", sizeof(s5gpu_diff_side_t));return 0;}\n'
    src.write_text(text)
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "d")])
    lines = subprocess.check_output([str(tmp_path / "d")], text=True).split("\n")
    for line, dt, size in zip(lines, (_lib.SIG_DIFF, _lib.DIFF_ACC), (80, 1048696)):
        got = [int(v) for v in line.split()]
        assert got[0] == dt.itemsize == size and got[1:] == [dt.fields[n][1] for n in dt.names]
    assert int(lines[2]) == C.sizeof(_lib.DiffSide)
    assert _lib.lib().s5gpu_diff_acc_bytes() == 1048696


def test_the_oracle_on_a_hand_made_case():
    a = Read(b"r", 0, DOUBLES, [5, -3, 7, 7, 100], b"x")
    b = Read(b"r", 0, DOUBLES, [5, 1, 3, 11], b"x")
    r = pair_ref(a, b)
    assert (r["n_a"], r["n_b"], r["flags"], r["n_diff"], r["first_diff"], r["max_abs"], r["max_at"]) == (5, 4, SIGNAL | LEN, 3, 1, 4, 1)
    assert (r["sum_d"], r["sum_abs"], r["sum_sq"], r["sum_a"], r["sumsq_a"]) == (4, 12, 48, 16, 25 + 9 + 49 + 49)
    o = acc_ref([r, failed_row(2, 0)], [diff_of(a, b)])
    assert (o["n_pairs"], o["n_failed"], o["n_differ"], o["n_signal"], o["n_len"], o["n_samples"], o["n_diff"], o["max_abs"]) == (2, 1, 1, 1, 1, 4, 3, 4)
    assert o["hist"][65535] == 1 and o["hist"][65535 + 4] == 2 and o["hist"][65535 - 4] == 1 and o["hist"].sum() == 4


# tests/golden/ref/raw/degrade/X.blow5 against ref/exp/degrade/X_bN.blow5: (X, bits, reads, samples, n_diff, max_abs)
DEGRADE = [("gridr10dna", 3, 8, 458496, 401164, 4), ("minir10dna", 3, 8, 458496, 401164, 4), ("promr10dna4khz", 3, 8, 458496, 401164, 4),
           ("promr10dna5khz", 3, 8, 458496, 401164, 4), ("PRPN119035_read1", 2, 1, 49691, 38486, 2),
           ("na12878_prom_merged_r9.4.1_chr22_read1", 2, 1, 146215, 116999, 2), ("p2solo_ulk114_dna", 3, 1, 2050027, 1829622, 4),
           ("promr10rna", 3, 8, 458496, 0, 0)]
_REF = {}


def degrade_paths(x, bits):
    return golden("ref/raw/degrade/%s.blow5" % x), golden("ref/exp/degrade/%s_b%d.blow5" % (x, bits))


def file_pair_ref(path_a, path_b):
    """the oracle of a file pair, computed once: dict(ids, rows, ds, acc, only_a, only_b, fa, fb); the pairs in A's order"""
    key = (path_a, path_b)
    if key not in _REF:
        ra, fa = file_reads(path_a)
        rb, fb = file_reads(path_b)
        by_id = {r.rid: r for r in rb}
        assert len(by_id) == len(rb)
        paired = [(a, by_id[a.rid]) for a in ra if a.rid in by_id]
        rows = [pair_ref(a, b) for a, b in paired]
        ds = [diff_of(a, b) for a, b in paired]
        ida = {a.rid for a in ra}
        _REF[key] = dict(ids=[a.rid for a, _ in paired], rows=rows, ds=ds, acc=acc_ref(rows, ds), fa=fa, fb=fb,
                         only_a=sorted(a.rid for a in ra if a.rid not in by_id), only_b=sorted(b.rid for b in rb if b.rid not in ida),
                         same_order=[a.rid for a in ra] == [b.rid for b in rb])
    return _REF[key]


@pytest.mark.parametrize("x,bits,reads,samples,n_diff,max_abs", DEGRADE)
def test_the_rule_on_the_reference_degrade_pairs(x, bits, reads, samples, n_diff, max_abs):
    ref = file_pair_ref(*degrade_paths(x, bits))
    acc = ref["acc"]
    assert ref["same_order"] and not ref["only_a"] and not ref["only_b"]
    assert (acc["n_pairs"], acc["n_samples"], acc["n_diff"], acc["max_abs"]) == (reads, samples, n_diff, max_abs)
    assert all(int(r["flags"]) == (SIGNAL if r["n_diff"] else 0) for r in ref["rows"])         # no field, aux or length difference
    assert ref["fa"].sig_method == ob.SIG_SVB_ZD and ref["fb"].sig_method == (ob.SIG_SVB_ZD if x == "promr10dna4khz" else ob.SIG_EX_ZD)
    assert ref["fa"].rec_method == ref["fb"].rec_method == ob.REC_ZLIB
    # B is A rounded at `bits` bits (the restated rule of §4.8)
    ra, _ = file_reads(degrade_paths(x, bits)[0])
    assert all(np.array_equal(d, qts(a.sig, bits).astype(np.int64) - a.sig) for a, d in zip(ra, ref["ds"]))


# ---------------------------------------------------------------------------------------------------------------- gpu

@pytest.fixture(scope="module")
def gpu():
    import torch
    from slow5tools_amd import _lib, diff, press

    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.diff, env.press = torch, _lib, _lib.lib(), diff, press
    return env


DEFAULTS = dict(lds_bins=64, flush_samples=0xFFFFFFFF, grid=1024)


@pytest.fixture
def options(gpu):
    def set_(**kw):
        for k, v in kw.items():
            gpu.lib.check(gpu.L.s5gpu_set_option(("diff_" + k).encode(), v), k)

    yield set_
    set_(**DEFAULTS)


def assert_rows(got, want, names):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, names):
        assert_same(g, w, name)


@pytest.mark.gpu
def test_every_crafted_pair_through_the_handle(gpu, crafted):
    """zlib + svb-zd on side A against zlib + ex-zd on side B, one batch: every row and the accumulator, the 131 071 bins included"""
    rows, acc = gpu.diff.pair_diffs(crafted.stored_a, (ob.REC_ZLIB, ob.SIG_SVB_ZD), crafted.stored_b, (ob.REC_ZLIB, ob.SIG_EX_ZD))
    assert_rows(rows, crafted.rows, [w for w, _a, _b in crafted.pairs])
    assert_same(acc, acc_ref(crafted.rows, crafted.ds), "one batch")


PRESS_PICK = ["identical 0", "random 9", "rounded at 3 bits 513", "a longer 4097", "aux of different lengths", "0.0 against -0.0", "random 4000"]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(9))
def test_each_press_pair_against_a_rotated_one(gpu, crafted, k):
    pa, pb = PRESSES[k], PRESSES[(k + 4) % 9]
    idx = [i for i, (w, _a, _b) in enumerate(crafted.pairs) if w in PRESS_PICK]
    assert len(idx) == len(PRESS_PICK)
    rows, acc = gpu.diff.pair_diffs([crafted.pairs[i][1].stored(*pa) for i in idx], pa, [crafted.pairs[i][2].stored(*pb) for i in idx], pb)
    want, ds = crafted.subset(idx)
    assert_rows(rows, want, [crafted.pairs[i][0] for i in idx])
    assert_same(acc, acc_ref(want, ds), "%r against %r" % (pa, pb))


def dev_pick(crafted):
    return [i for i, (w, _a, _b) in enumerate(crafted.pairs)
            if w.split(" ")[-1] in ("0", "9", "513", "2049") or not w[-1].isdigit() or w.startswith("aux of 700")]


def decode_both(gpu, crafted, idx, no_payload):
    kw = dict(no_payload=no_payload)
    if not no_payload:
        kw["max_pay_cap"] = 16384
    a = gpu.press.decode_to_device([crafted.stored_a[i] for i in idx], ob.REC_ZLIB, ob.SIG_SVB_ZD, **kw)
    b = gpu.press.decode_to_device([crafted.stored_b[i] for i in idx], ob.REC_ZLIB, ob.SIG_EX_ZD, **kw)
    return a, b


@pytest.mark.gpu
def test_signal_diff_dev_over_two_device_decodes(gpu, crafted):
    """permuted, repeated and out-of-range pair indices; with the payloads and without; rows and accumulator between guard words"""
    torch, L, lib = gpu.torch, gpu.L, gpu.lib
    idx = dev_pick(crafted)
    n = len(idx)
    assert n > 60
    rng = np.random.default_rng(9)
    pa = np.concatenate([rng.permutation(n), rng.integers(0, n, size=40), [n, 0, 0xFFFFFFFF, 3]]).astype(np.uint32)
    pb = np.concatenate([pa[:n], rng.integers(0, n, size=40), [0, n + 7, 5, 0x80000000]]).astype(np.uint32)
    for payload in (True, False):
        da, db = decode_both(gpu, crafted, idx, no_payload=not payload)
        want, ds = [], []
        for ia, ib in zip(pa, pb):
            if ia >= n or ib >= n:
                want.append(failed_row(0, 0, BAD_PAIR))
            else:
                a, b = crafted.pairs[idx[ia]][1], crafted.pairs[idx[ib]][2]
                want.append(pair_ref(a, b, payload=payload))
                ds.append(diff_of(a, b))
        assert sum(1 for r in want if r["flags"] == BAD_PAIR) == 4
        if not payload:
            assert not any(int(r["flags"]) & (ID | AUX) for r in want)
        acc = gpu.diff.new_acc()
        rows = gpu.diff.diff_dev(da, db, pa, pb, acc, payload=payload)
        assert_rows(rows, want, ["pair %d (%d, %d) payload=%s" % (p, ia, ib, payload) for p, (ia, ib) in enumerate(zip(pa, pb))])
        assert_same(gpu.diff.to_numpy(acc), acc_ref(want, ds), "payload=%s" % payload)
        assert gpu.diff.diff_dev(da, db, pa, pb, None, payload=payload, want_rows=True).tobytes() == rows.tobytes()      # acc may be NULL
    # guard words before and after out and acc; out == NULL
    dev = da.dev
    G, words, m = 8, lib.DIFF_ACC.itemsize // 8, len(pa)
    t_acc = torch.from_numpy(np.full(G + words + G, GUARD, dtype=np.uint64).view(np.int64)).to(dev)
    t_out = torch.from_numpy(np.full(G + 10 * m + G, GUARD, dtype=np.uint64).view(np.int64)).to(dev)
    A, B = gpu.diff._Side(da, False), gpu.diff._Side(db, False)
    t_pa, t_pb = (torch.from_numpy(p.view(np.int32).copy()).to(dev) for p in (pa, pb))
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    acc_p, out_p = t_acc.data_ptr() + 8 * G, t_out.data_ptr() + 8 * G
    lib.check(L.s5gpu_diff_acc_reset_dev(acc_p, st), "reset")
    lib.check(L.s5gpu_signal_diff_dev(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), out_p, acc_p, st), "diff")
    lib.check(L.s5gpu_signal_diff_dev(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), None, acc_p, st), "diff without rows")
    torch.cuda.synchronize(dev)
    h, o = t_acc.cpu().numpy().view(np.uint64), t_out.cpu().numpy().view(np.uint64)
    assert (h[:G] == GUARD).all() and (h[G + words:] == GUARD).all() and (o[:G] == GUARD).all() and (o[G + 10 * m:] == GUARD).all()
    assert o[G:G + 10 * m].tobytes() == rows.tobytes()
    twice = acc_ref(want + want, ds + ds)
    assert_same(h[G:G + words].view(lib.DIFF_ACC)[0], twice, "two launches into one accumulator")
    # refused arguments: nothing is launched
    call = lambda *a: L.s5gpu_signal_diff_dev(*a)
    assert call(m, None, t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), out_p, acc_p, st) == -1
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), None, C.byref(B.c), out_p, acc_p, st) == -1
    assert call(m, t_pa.data_ptr() + 2, t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), out_p, acc_p, st) == -1
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), out_p + 4, acc_p, st) == -1
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(A.c), C.byref(B.c), out_p, acc_p + 4, st) == -1
    bad = gpu.diff._Side(da, False)
    bad.c.sig = da.t_sig.data_ptr() + 2
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(bad.c), C.byref(B.c), out_p, acc_p, st) == -1
    bad.c.sig, bad.c.fields = da.t_sig.data_ptr(), None
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(A.c), C.byref(bad.c), out_p, acc_p, st) == -1
    bad = gpu.diff._Side(da, False)
    bad.c.payload = da.t_scr.data_ptr()                              # a payload without its offsets
    assert call(m, t_pa.data_ptr(), t_pb.data_ptr(), C.byref(bad.c), C.byref(B.c), out_p, acc_p, st) == -1
    assert L.s5gpu_diff_acc_reset_dev(None, st) == -1 and L.s5gpu_diff_acc_reset_dev(acc_p + 4, st) == -1
    assert call(0, None, None, None, None, None, None, st) == 0
    torch.cuda.synchronize(dev)
    assert (t_acc.cpu().numpy().view(np.uint64) == h).all()


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["a", "b"])
def test_a_corrupt_and_a_truncated_record_between_good_ones(gpu, crafted, side):
    """beside a long constant read whose payload outgrows the slot the decoder guesses for it, so that the batch is decoded again without
    the corrupt records"""
    names = ["random 513", "rounded at 3 bits 4000", "+1 everywhere 2049", "a longer 4097", "random 65", "identical 9"]
    idx = [[k for k, (w, _a, _b) in enumerate(crafted.pairs) if w == name][0] for name in names]
    const = np.full(60000, 517, dtype=np.int16)
    ca, cb = Read(b"long-constant", 1, DOUBLES, const), Read(b"long-constant", 1, DOUBLES, (const + 2).astype(np.int16))
    sa = [crafted.stored_a[i] for i in idx] + [ca.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD)]
    sb = [crafted.stored_b[i] for i in idx] + [cb.stored(ob.REC_ZLIB, ob.SIG_EX_ZD)]
    hurt = sa if side == "a" else sb
    flipped = bytearray(hurt[1])
    flipped[len(flipped) // 2] ^= 0x5A
    hurt[1] = bytes(flipped)
    hurt[3] = hurt[3][:len(hurt[3]) // 2]
    h = gpu.diff.Handle()
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        h.add(sa, (ob.REC_ZLIB, ob.SIG_SVB_ZD), sb, (ob.REC_ZLIB, ob.SIG_EX_ZD))
    rows2, st_a2, st_b2 = h.add(sa[:1] + sa[4:], (ob.REC_ZLIB, ob.SIG_SVB_ZD), sb[:1] + sb[4:], (ob.REC_ZLIB, ob.SIG_EX_ZD))     # the handle still works
    assert not st_a2.any() and not st_b2.any()
    good = [0, 2, 4, 5]
    want = [crafted.rows[idx[k]] for k in good] + [pair_ref(ca, cb)]
    ds = [crafted.ds[idx[k]] for k in good] + [diff_of(ca, cb)]
    again = [want[0], want[2], want[3], want[4]]
    assert_rows(rows2, again, ["second batch"] * 4)
    acc = h.close()
    assert acc["n_failed"] == 2 and acc["n_pairs"] == 11
    assert_same(acc, acc_ref(want + [failed_row(1, 0), failed_row(1, 0)] + again, ds + [ds[0], ds[2], ds[3], ds[4]]), "past the corrupt records")
    # the rows of the failed call
    h = gpu.diff.Handle()
    rows, st_a, st_b = h.add(sa, (ob.REC_ZLIB, ob.SIG_SVB_ZD), sb, (ob.REC_ZLIB, ob.SIG_EX_ZD), raise_on_error=False)
    h.abandon()
    st_hurt, st_other = (st_a, st_b) if side == "a" else (st_b, st_a)
    assert st_hurt[1] != 0 and st_hurt[3] != 0 and not np.delete(st_hurt, [1, 3]).any() and not st_other.any()
    for k in (1, 3):
        assert_same(rows[k], failed_row(st_a[k], st_b[k]), "the failed pair %d" % k)
    assert_rows([rows[k] for k in good] + [rows[6]], want, ["neighbour"] * 5)


@pytest.mark.gpu
def test_the_accumulator_under_every_option(gpu, crafted, options):
    idx = dev_pick(crafted) + crafted.extreme[:6]
    da, db = decode_both(gpu, crafted, idx, no_payload=True)
    n = len(idx)
    ident = np.arange(n, dtype=np.uint32)
    rows, ds = [pair_ref(crafted.pairs[i][1], crafted.pairs[i][2], payload=False) for i in idx], [crafted.ds[i] for i in idx]
    want = acc_ref(rows, ds)
    assert want["hist"][0] > 0 and want["hist"][131070] > 0 and want["hist"][65535 + 4] > 0 and want["hist"][65535 + 1] > 0      # ±65535 next to small differences

    def run(pairs=ident):
        acc = gpu.diff.new_acc()
        gpu.diff.diff_dev(da, db, pairs, pairs, acc, want_rows=False)
        return gpu.diff.to_numpy(acc)

    for what, kw in (("the defaults", dict()), ("no LDS bins", dict(lds_bins=0)), ("the smallest window", dict(lds_bins=8)), ("the largest window", dict(lds_bins=256)),
                     ("one workgroup walks every pair", dict(grid=1)), ("two workgroups", dict(grid=2)),
                     ("one workgroup, a flush every 300 samples", dict(grid=1, flush_samples=300)),
                     ("two workgroups, a flush every 1000 samples, smallest window", dict(grid=2, flush_samples=1000, lds_bins=8)),
                     ("three workgroups, no LDS bins", dict(grid=3, lds_bins=0)), ("a flush before every pair", dict(grid=5, flush_samples=1))):
        options(**DEFAULTS)
        options(**kw)
        assert_same(run(), want, what)
    # Every difference inside the window.  The window is fixed around 0 and has at most 256 bins, d = -128 .. 127, so this run cannot hold
    # the pairs of d = +-65535, and neither the random pairs nor those rounded at 16 bits, whose differences span thousands of values: no
    # LDS window can.  What is left out is exactly these three kinds (asserted), and every other pair of the batch is in.
    inside = [k for k in range(n) if rows[k]["max_abs"] <= 127]
    left_out = [crafted.pairs[idx[k]][0] for k in range(n) if k not in inside]
    assert len(left_out) == 12 + 3 + 3 and all(w.startswith(("d = ", "random ", "rounded at 16 bits ")) for w in left_out), left_out
    want_in = acc_ref([rows[k] for k in inside], [ds[k] for k in inside])
    for kw in (dict(lds_bins=256), dict(lds_bins=256, grid=1, flush_samples=500), dict(lds_bins=256, grid=2)):
        options(**DEFAULTS)
        options(**kw)
        assert_same(run(np.array(inside, dtype=np.uint32)), want_in, "every difference inside the window %r" % (kw,))
    # one batch against the same pairs cut into three batches
    options(**DEFAULTS)
    acc = gpu.diff.new_acc()
    for part in np.array_split(ident, 3):
        gpu.diff.diff_dev(da, db, part, part, acc, want_rows=False)
    assert_same(gpu.diff.to_numpy(acc), want, "three launches")
    # ... and through the handle, with the payloads
    sa, sb = [crafted.stored_a[i] for i in idx], [crafted.stored_b[i] for i in idx]
    full = acc_ref([crafted.rows[i] for i in idx], ds)
    for batch in (None, (n + 2) // 3):
        rows_h, acc_h = gpu.diff.pair_diffs(sa, (ob.REC_ZLIB, ob.SIG_SVB_ZD), sb, (ob.REC_ZLIB, ob.SIG_EX_ZD), batch=batch)
        assert_rows(rows_h, [crafted.rows[i] for i in idx], ["handle"] * n)
        assert_same(acc_h, full, "handle, batch=%r" % batch)


# ---------------------------------------------------------------------------------------------------------------- the tool

def s5diff(*args):
    return subprocess.run([S5DIFF] + [str(a) for a in args], capture_output=True, timeout=300)


def header_line(text, prefix):
    found = [l for l in text.split(b"\n") if l.startswith(prefix)]
    return found[0] if found else None


def expected_text(path_a, path_b):
    """what `s5diff a b` prints, formatted from the oracle's numbers; and whether any pair is flagged or unpaired"""
    ref = file_pair_ref(path_a, path_b)
    out = [b"#s5diff\t1\n"]
    ha, hb = xxh64(ref["fa"].header_text), xxh64(ref["fb"].header_text)
    if ha != hb:
        out.append(b"header\t%016x\t%016x\n" % (ha, hb))
    layout = any(header_line(ref["fa"].header_text, p) != header_line(ref["fb"].header_text, p) for p in (b"#char*", b"#read_id"))
    if layout:
        out.append(b"aux-layout\n")
    flagged = 0
    for rid, r in zip(ref["ids"], ref["rows"]):
        fl = int(r["flags"]) & (~AUX if layout else ~0)
        if not fl:
            continue
        flagged += 1
        n = min(int(r["n_a"]), int(r["n_b"]))
        dash = lambda v: b"-" if v == NONE else b"%d" % v
        rmse = (b"%.6g" % math.sqrt(float(int(r["sum_sq"])) / n)) if n else b"-"
        out.append(b"\t".join([rid, b",".join(FLAG_NAMES[k].encode() for k in range(9) if fl >> k & 1), b"%d" % r["n_a"], b"%d" % r["n_b"], b"%d" % r["n_diff"],
                               dash(r["first_diff"]), b"%d" % r["max_abs"], dash(r["max_at"]), rmse]) + b"\n")
    for rid, which in sorted([(i, b"only-in-a") for i in ref["only_a"]] + [(i, b"only-in-b") for i in ref["only_b"]]):
        out.append(which + b"\t" + rid + b"\n")
    acc = ref["acc"]
    out.append(b"#pairs\t%d\t%d\n#samples\t%d\t%d\n#max_abs\t%d\n#sum_abs\t%d\n#sum_sq\t%d\n" % (len(ref["rows"]), flagged, acc["n_samples"], acc["n_diff"],
                                                                                                    acc["max_abs"], acc["sum_abs"], acc["sum_sq"]))
    out.append(b"#rmse\t%.6g\n" % math.sqrt(float(int(acc["sum_sq"])) / int(acc["n_samples"])) if acc["n_samples"] else b"#rmse\t-\n")
    out.append(b"#snr_db\t%.4f\n" % (10.0 * math.log10(float(int(acc["sumsq_a"])) / float(int(acc["sum_sq"])))) if acc["sum_sq"] else b"#snr_db\tinf\n")
    return b"".join(out), bool(flagged or ref["only_a"] or ref["only_b"])


@pytest.mark.gpu
@pytest.mark.parametrize("x,bits", [(d[0], d[1]) for d in DEGRADE])
def test_s5diff_on_the_reference_degrade_pairs(gpu, x, bits, tmp_path):
    a, b = degrade_paths(x, bits)
    want, differs = expected_text(a, b)
    p = s5diff("--hist", tmp_path / "h.tsv", a, b)
    assert p.stdout == want, p.stderr
    assert p.returncode == (1 if differs else 0)
    hist = file_pair_ref(a, b)["acc"]["hist"]
    assert open(tmp_path / "h.tsv").read() == "".join("%d\t%d\n" % (k - 65535, hist[k]) for k in np.nonzero(hist)[0])
    assert s5diff("--tol", 1 << (bits - 1), a, b).returncode == 0 and s5diff("--tol", 1 << (bits - 1), a, b).stdout == want
    if differs:
        assert s5diff("--tol", (1 << (bits - 1)) - 1, a, b).returncode == 1


@pytest.mark.gpu
def test_s5diff_tolerance_batches_and_the_projects_own_degrade(gpu, tmp_path):
    a, b = degrade_paths("gridr10dna", 3)
    assert s5diff("--tol", 4, a, b).returncode == 0 and s5diff("--tol", 3, a, b).returncode == 1
    outs = [s5diff("-K", k, a, b) for k in (1, 3, 4096)]
    assert outs[0].stdout == outs[1].stdout == outs[2].stdout == expected_text(a, b)[0] and all(o.returncode == 1 for o in outs)
    mine = tmp_path / "mine_b3.blow5"
    r = subprocess.run([S5VIEW, "--degrade", "3", a, str(mine)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    p = s5diff("--tol", 4, a, mine)
    assert p.returncode == 0 and p.stdout == expected_text(a, str(mine))[0], p.stderr
    assert s5diff(a, mine).returncode == 1
    res = gpu.diff.file_diff(a, b, batch=5, tol=4)
    assert res["exit"] == 0 and len(res["pairs"]) == 8 and res["summary"]["samples"] == ["458496", "401164"] and res["pairs"][0]["flags"] == "signal"


LOSSLESS = ["exp_1_lossless.blow5", "exp_1_lossless_v0.2.0.blow5", "exp_1_lossless_zlib.blow5", "exp_1_lossless_zlib_ex_zd.blow5",
            "exp_1_lossless_zlib_svb_v0.2.0.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5", "exp_1_lossless_zstd_v0.2.0.blow5"]
MULTI = ["example_multi_rg_v0.1.0.blow5", "example_multi_rg_v0.2.0.blow5", "example_multi_rg_v0.2.0_zstd_svb-zd.blow5"]


@pytest.mark.gpu
@pytest.mark.parametrize("first,name", [(LOSSLESS[0], n) for n in LOSSLESS[1:]] + [(LOSSLESS[3], LOSSLESS[0])] + [(MULTI[0], n) for n in MULTI[1:]] + [(MULTI[2], MULTI[1])])
def test_s5diff_on_the_lossless_families(gpu, first, name):
    a, b = golden(first), golden(name)
    p = s5diff(a, b)
    want, differs = expected_text(a, b)
    assert p.returncode == 0 and not differs and p.stdout == want, (name, p.stderr)
    assert not [l for l in p.stdout.split(b"\n") if l and not l.startswith((b"#", b"header\t"))]


@pytest.mark.gpu
def test_s5diff_on_a_lossy_twin_and_on_reversed_records(gpu, tmp_path):
    # the lossy twin has no aux fields: the headers' aux lines differ
    a, b = golden("exp_1_lossless.blow5"), golden("ref/exp/one_fast5/exp_1_lossy.blow5")
    p = s5diff(a, b)
    want, _ = expected_text(a, b)
    assert p.stdout == want and b"aux-layout\n" in p.stdout, p.stderr
    assert file_pair_ref(a, b)["rows"][0]["flags"] & AUX            # the kernel's flag, masked by the tool
    # the records reversed
    f = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    body = b"".join(f.raw[o:o + 8 + len(r)] for o, r in reversed(list(zip(f.offsets, f.records))))
    (tmp_path / "reversed.blow5").write_bytes(f.raw[:f.offsets[0]] + body + b"5WOLB")
    p = s5diff(golden("example_multi_rg_v0.2.0.blow5"), tmp_path / "reversed.blow5")
    assert p.returncode == 0 and p.stdout == expected_text(golden("example_multi_rg_v0.2.0.blow5"), str(tmp_path / "reversed.blow5"))[0], p.stderr


@pytest.mark.gpu
def test_s5diff_unpaired_ids_and_errors(gpu, tmp_path):
    a, b = golden("example_multi_rg_v0.2.0.blow5"), golden("ref/exp/get/expected_extracted_reads.blow5")
    p = s5diff(a, b)
    want, _ = expected_text(a, b)
    lines = [l for l in p.stdout.split(b"\n") if l and not l.startswith((b"#", b"header\t", b"aux-layout"))]
    assert p.returncode == 1 and p.stdout == want and lines and all(l.startswith((b"only-in-a\t", b"only-in-b\t")) for l in lines), p.stderr
    assert b"#pairs\t0\t0\n" in p.stdout and b"#rmse\t-\n" in p.stdout
    dup = golden("ref/exp/index/duplicate_read.blow5")
    for x, y in ((dup, a), (a, dup), (dup, dup)):
        p = s5diff(x, y)
        assert p.returncode == 2 and b"more than once" in p.stderr and p.stdout == b""
    p = s5diff(golden("exp_1_lossless.slow5"), golden("exp_1_lossless.blow5"))
    assert p.returncode == 2 and b"convert" in p.stderr
    p = s5diff(golden("exp_1_lossless.blow5"), golden("exp_1_lossless.slow5"))
    assert p.returncode == 2 and b"convert" in p.stderr
    assert s5diff(golden("no_such_file.blow5"), a).returncode == 2 and s5diff(a).returncode == 2 and s5diff("--tol", "x", a, a).returncode == 2
    # a corrupt record
    f = Blow5(a)
    raw = bytearray(f.raw)
    raw[f.offsets[2] + 8 + len(f.records[2]) // 2] ^= 0x5A
    (tmp_path / "bad.blow5").write_bytes(bytes(raw))
    p = s5diff(a, tmp_path / "bad.blow5")
    assert p.returncode == 2 and p.stdout == b"" and b"corrupt" in p.stderr
