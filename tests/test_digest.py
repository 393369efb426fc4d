"""sum: per-read content digests hashed on the device (k_rec_digest), the three C calls, slow5tools_amd.digest and the s5sum tool.

The oracle is digest_ref in this file: the canonical record C(r) (docs/codecs.md §4.12) rebuilt on the CPU from the stored record with the
oracle's decoders (zlib, the image's libzstd or the oracle's restated zstd decoder, oracle_bind's svb-zd / ex-zd decoders) and hashed with
zstd_craft.xxh64.  Every comparison is exact.

  not gpu : exported symbols and bindings; xxh64's empty-input value; the digests the definition was checked with on the reference's own files.
  gpu     : crafted records of every length class mod 32, every alignment of the signal and every press pair through s5gpu_digest_batch and
            s5gpu_digest_stream; corrupt and truncated records between good ones; s5gpu_digest_dev between guard words with a status-6 record;
            s5sum on every golden BLOW5 file, with several batch and chunk sizes, on a .slow5, and --compare; refused arguments.
"""
import ctypes as C
import hashlib
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
S5SUM = os.path.join(ROOT, "slow5tools_amd", "s5sum")
NAMES = ["s5gpu_digest_dev", "s5gpu_digest_stream", "s5gpu_digest_batch"]
PAIRS = [(r, s) for r in (ob.REC_NONE, ob.REC_ZLIB, ob.REC_ZSTD) for s in (ob.SIG_NONE, ob.SIG_SVB_ZD, ob.SIG_EX_ZD)]
GUARD = 0xA5A5A5A5A5A5A5A5


# ---------------------------------------------------------------------------------------------------------------- the oracle

def depress(rec, rec_method):
    """the uncompressed record of a stored one"""
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
        assert len(blob) == L
        sig = ob.svbzd_decode(blob) if sig_method == ob.SIG_SVB_ZD else ob.exzd_decode(blob)
        assert sig is not None
    assert hl + 8 + nb <= len(payload)
    return payload[:hl], np.asarray(sig, dtype=np.int16), payload[hl + 8 + nb:]


def canonical(payload, sig_method):
    """C(r): the record as a BLOW5 file with record press none and signal press none stores it, without the u64 size prefix"""
    head, sig, aux = pieces(payload, sig_method)
    return head + struct.pack("<Q", len(sig)) + sig.astype("<i2").tobytes() + aux


_HASHED = {}


def xxh64_once(b):
    """zstd_craft.xxh64, each distinct input hashed once (the golden families hold the same reads many times)"""
    k = hashlib.sha1(b).digest()
    if k not in _HASHED:
        _HASHED[k] = xxh64(b)
    return _HASHED[k]


def digest_ref(rec, rec_method, sig_method):
    return xxh64_once(canonical(depress(rec, rec_method), sig_method))


def file_ref(path):
    """(ids, digests) of a BLOW5 file in file order"""
    f = Blow5(path)
    ids, digs = [], []
    for r in f.records:
        c = canonical(depress(r, f.rec_method), f.sig_method)
        (idl,) = struct.unpack_from("<H", c, 0)
        ids.append(c[2:2 + idl])
        digs.append(xxh64_once(c))
    return ids, digs, f


def slow5_ref(path):
    """(ids, digests) of a SLOW5 ASCII file: every record line through the oracle's line parser"""
    text = open(path, "rb").read().split(b"\n")
    types = ob.aux_types([l for l in text if l.startswith(b"#char*")][0])
    ids, digs = [], []
    for l in text:
        if l and l[:1] not in b"#@":
            pay = ob.line_to_payload(l, types)
            assert pay is not None
            ids.append(l.split(b"\t", 1)[0])
            digs.append(xxh64_once(canonical(pay, ob.SIG_NONE)))
    return ids, digs


def sum_lines(path):
    """what `s5sum path` prints"""
    ids, digs, f = file_ref(path)
    out = [b"#s5sum\t1\txxh64\t%016x\n" % xxh64_once(f.header_text)]
    out += [b"%016x\t%s\n" % (d, i) for i, d in zip(ids, digs)]
    out.append(b"#total\t%d\t%016x\n" % (len(ids), sum(digs) & (2 ** 64 - 1)))
    return b"".join(out)


def all_blow5():
    """every BLOW5 file under tests/golden that blow5_fixture.Blow5 reads, grouped by content: byte-identical copies (the reference keeps the
    same file in several of its test directories) are one case, named after the first path"""
    groups = {}
    for d, _, fs in sorted(os.walk(GOLDEN)):
        for f in sorted(fs):
            if f.endswith(".blow5"):
                p = os.path.join(d, f)
                try:
                    Blow5(p)
                except Exception:
                    continue   # damaged on purpose (quickcheck's bad files)
                groups.setdefault(hashlib.sha1(open(p, "rb").read()).digest(), []).append(os.path.relpath(p, GOLDEN))
    return sorted(sorted(g)[0] for g in groups.values())


ALL = all_blow5()
DUPLICATE = "ref/exp/index/duplicate_read.blow5"


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_and_binds_the_digest_calls():
    from slow5tools_amd import _lib, digest

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in NAMES if s not in exported]
    assert not [s for s in NAMES if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert len(L.s5gpu_digest_dev.argtypes) == 8 and len(L.s5gpu_digest_stream.argtypes) == 9 and len(L.s5gpu_digest_batch.argtypes) == 7
    assert callable(digest.record_digests) and callable(digest.file_digests)
    assert os.access(S5SUM, os.X_OK)


def test_xxh64_of_nothing():
    assert xxh64(b"") == 0xEF46DB3751D8E999


LOSSLESS = ["exp_1_lossless.blow5", "exp_1_lossless_v0.2.0.blow5", "exp_1_lossless_zlib.blow5", "exp_1_lossless_zlib_ex_zd.blow5",
            "exp_1_lossless_zlib_svb_v0.2.0.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5", "exp_1_lossless_zstd_v0.2.0.blow5"]


@pytest.mark.parametrize("name", LOSSLESS)
def test_the_lossless_family_has_one_digest(name):
    ids, digs, f = file_ref(golden(name))
    assert digs == [0x4AE2FEF7913FAF61] and len(ids[0]) == 36


def test_the_slow5_line_has_the_same_digest():
    ids, digs = slow5_ref(golden("exp_1_lossless.slow5"))
    assert digs == [0x4AE2FEF7913FAF61] and ids == file_ref(golden("exp_1_lossless.blow5"))[0]


def test_the_other_families_agree_and_lossy_differs():
    multi = [file_ref(golden(n))[:2] for n in ("example_multi_rg_v0.1.0.blow5", "example_multi_rg_v0.2.0.blow5", "example_multi_rg_v0.2.0_zstd_svb-zd.blow5")]
    assert multi[0] == multi[1] == multi[2] and len(multi[0][1]) == 7
    assert multi[0][1][:2] == [0xA53243C665615CF0, 0x6E1E06718C6CD676]
    aux = [file_ref(golden(n))[1] for n in ("aux_array_exp_lossless.blow5", "exp_lossless_gzip.blow5")]
    assert aux[0] == aux[1] == [0xC12730225127091B]
    ssm = [file_ref(golden("ref/exp/f2s/multi-fast5-output/" + n))[:2] for n in ("ssm1_zlib.blow5", "ssm1_zlib_svb.blow5")]
    assert ssm[0] == ssm[1] and len(ssm[0][1]) > 0
    lossy = {file_ref(golden("ref/exp/one_fast5/" + n))[1][0] for n in os.listdir(golden("ref/exp/one_fast5")) if n.startswith("exp_1_lossy") and n.endswith(".blow5")}
    assert lossy == {0xAC1617E03EC409C2}                                   # the aux fields are gone: another digest
    # the header digest is the stored text's: the two exp_1_lossless files of one version share it
    assert xxh64_once(Blow5(golden("exp_1_lossless_v0.2.0.blow5")).header_text) == xxh64_once(Blow5(golden("exp_1_lossless_zstd_v0.2.0.blow5")).header_text)


# ---------------------------------------------------------------------------------------------------------------- crafted records

NS = [0, 1, 2, 3, 4, 11, 12, 13, 15, 16, 17, 255, 4000, 4097, 70001]
# 38 + id_len is where the N word begins and 46 + id_len where the signal does: 6 and 8 complete the signal's alignments mod 8 (4 and 6)
ID_LENS = [1, 2, 35, 36, 37, 43, 255, 6, 8]
AUX_LENS = [0, 1, 7, 8, 31, 32, 33]
KINDS = ["random", "constant", "alternating", "lowest"]


def _contents(n, kind, rng):
    if kind == "random":
        return rng.integers(-32768, 32768, size=n, dtype=np.int32).astype(np.int16)
    if kind == "constant":
        return np.full(n, 517, dtype=np.int16)
    if kind == "alternating":
        return np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
    return np.full(n, -32768, dtype=np.int16)


def crafted_plan():
    """(N, id_len, aux_len, kind): every id length x aux length for the short reads, every id length with the aux lengths in turn for the long"""
    plan = []
    for j, n in enumerate(NS):
        for a, idl in enumerate(ID_LENS):
            auxs = AUX_LENS if n <= 255 else [AUX_LENS[(a + j) % len(AUX_LENS)]]
            for ax in auxs:
                plan.append((n, idl, ax, KINDS[len(plan) % len(KINDS)]))
    return plan


class Crafted:
    def __init__(self):
        rng = np.random.default_rng(20)
        self.plan = crafted_plan()
        self.recs, self.keep, self.canon = [], [], []
        for k, (n, idl, ax, kind) in enumerate(self.plan):
            rid = bytes(rng.integers(0x21, 0x7F, size=idl, dtype=np.uint8))
            aux = bytes(rng.integers(0, 256, size=ax, dtype=np.uint8))
            sig = _contents(n, kind, rng)
            r, keep = ob.make_rec(rid, k % 5, 8192.0, 23.0 + k, 1467.61, 4000.0, sig, aux)
            self.recs.append(r)
            self.keep.append(keep)
            c = struct.pack("<H", idl) + rid + struct.pack("<Idddd", k % 5, 8192.0, 23.0 + k, 1467.61, 4000.0) + struct.pack("<Q", n) + sig.astype("<i2").tobytes() + aux
            assert len(c) == 2 + idl + 36 + 8 + 2 * n + ax
            self.canon.append(c)
        self.ref = np.array([xxh64(c) for c in self.canon], dtype=np.uint64)

    def stored(self, rec_method, sig_method, which=None):
        """the records (all, or those of the indices `which`) as a file with this press pair stores them (without the u64 prefix)"""
        out = []
        for r in self.recs if which is None else [self.recs[k] for k in which]:
            if rec_method == ob.REC_ZSTD:
                pay = ob.rec_pack(r, sig_method)
                out.append(ob.zstd_compress(pay) if ob.zstd_ref() else ob.zstd_literals_compress(pay))
            else:
                out.append(ob.rec_to_mem(r, rec_method, sig_method)[8:])
        return out


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


def test_the_crafted_set_covers_every_length_class_and_boundary(crafted):
    """asserted on the CPU, before any GPU test relies on it"""
    hl = np.array([38 + idl for _, idl, _, _ in crafted.plan])
    n2 = np.array([2 * n for n, _, _, _ in crafted.plan])
    ax = np.array([a for _, _, a, _ in crafted.plan])
    total = hl + 8 + n2 + ax
    assert [len(c) for c in crafted.canon] == total.tolist()
    assert set((total % 32).tolist()) == set(range(32))
    assert set(((hl + 8) % 8).tolist()) == set(range(8))                    # the signal's first byte at every alignment
    # each boundary between two pieces falls inside a 32-byte stripe and inside an 8-byte lane word, in a record long enough to have that
    # stripe (header | N at hl; N | signal at hl + 8; signal | aux at hl + 8 + 2N, with samples in front and aux bytes behind)
    for name, b, ok in (("header|N", hl, total >= 0), ("N|signal", hl + 8, n2 > 0), ("signal|aux", hl + 8 + n2, (n2 > 0) & (ax > 0))):
        in_stripe = ok & (b % 32 != 0) & (b // 32 < total // 32)
        in_word = ok & (b % 8 != 0) & (b // 32 < total // 32)
        in_tail = ok & (b % 8 != 0) & (b // 32 == total // 32) & (b < total)    # ... and inside a word of the tail behind the last stripe
        assert in_stripe.any() and in_word.any() and in_tail.any(), name
        assert set((b[in_word] % 8).tolist()) >= {1, 3, 5, 7}, name         # odd bytes included
    assert (total < 64).any() and (total > 2 ** 17).any()                   # one stripe only (a record cannot be shorter than 46 bytes); thousands
    # the reference hash of a record does not depend on how it is stored: every press pair decodes to the same canonical bytes
    which = list(range(0, len(crafted.plan), 61)) + [len(crafted.plan) - 1]
    for rec_method, sig_method in PAIRS:
        for k, rec in zip(which, crafted.stored(rec_method, sig_method, which)):
            assert canonical(depress(rec, rec_method), sig_method) == crafted.canon[k], (rec_method, sig_method, crafted.plan[k])


@pytest.fixture(scope="module")
def gpu():
    import torch
    from slow5tools_amd import _lib, digest, press

    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.digest, env.press = torch, _lib, _lib.lib(), digest, press
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("rec_method,sig_method", PAIRS)
def test_crafted_records_through_batch_and_stream(gpu, crafted, rec_method, sig_method):
    recs = crafted.stored(rec_method, sig_method)
    for k in range(0, len(recs), 97):                                        # the stored form decodes to the canonical bytes (CPU)
        assert canonical(depress(recs[k], rec_method), sig_method) == crafted.canon[k]
    for via in ("batch", "stream"):
        got, st = gpu.digest.record_digests(recs, rec_method, sig_method, raise_on_error=False, via=via)
        assert not st.any(), (via, np.nonzero(st)[0][:8], st[st != 0][:8])
        bad = np.nonzero(got != crafted.ref)[0]
        assert bad.size == 0, (via, [crafted.plan[i] for i in bad[:8]], len(bad))
    perm = np.random.default_rng(3).permutation(len(recs))
    got = gpu.digest.record_digests([recs[i] for i in perm], rec_method, sig_method, via="batch")
    assert np.array_equal(got, crafted.ref[perm])


@pytest.mark.gpu
@pytest.mark.parametrize("via", ["batch", "stream"])
def test_corrupt_and_truncated_records_between_good_ones(gpu, crafted, via):
    """a flipped byte inside a zlib stream and a truncated record: the call fails with S5GPU_ERR_DATA, those two have a status and digest 0,
    every other digest is right — a long constant read among them, whose payload outgrows the slot the decoder guessed for it"""
    long_const = [k for k, (n, _, _, kind) in enumerate(crafted.plan) if n == 70001 and kind == "constant"][0]
    pick = [k for k, (n, _, _, _) in enumerate(crafted.plan) if n in (13, 4000)][:9] + [long_const]
    batch = crafted.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD, pick)
    want = crafted.ref[pick].copy()
    flipped = bytearray(batch[2])
    flipped[len(flipped) // 2] ^= 0x5A
    batch[2] = bytes(flipped)
    batch[6] = batch[6][: len(batch[6]) // 2]
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        gpu.digest.record_digests(batch, ob.REC_ZLIB, ob.SIG_SVB_ZD, via=via)
    got, st = gpu.digest.record_digests(batch, ob.REC_ZLIB, ob.SIG_SVB_ZD, raise_on_error=False, via=via)
    for i in range(len(batch)):
        if i in (2, 6):
            assert st[i] != 0 and got[i] == 0, (i, st[i], got[i])
        else:
            assert st[i] == 0 and got[i] == want[i], (i, st[i], crafted.plan[pick[i]])


@pytest.mark.gpu
def test_digest_dev_over_a_device_decode_between_guard_words(gpu, crafted):
    torch, L = gpu.torch, gpu.L
    pick = [k for k, (n, idl, _, _) in enumerate(crafted.plan) if n in (3, 17, 255, 4000) and idl in (35, 36, 37)]
    recs = crafted.stored(ob.REC_ZLIB, ob.SIG_EX_ZD, pick)
    caps = [max(crafted.plan[k][0], 1) + (i % 3) for i, k in enumerate(pick)]
    small = [i for i, k in enumerate(pick) if crafted.plan[k][0] == 4000][0]
    caps[small] = 96                                                         # this record's signal does not fit: status 6
    dec = gpu.press.decode_to_device(recs, ob.REC_ZLIB, ob.SIG_EX_ZD, max_pay_cap=48 * 1024, sig_caps=caps, no_payload=False)
    f = dec.t_fields.cpu().numpy().view(gpu.lib.REC_FIELDS)[:len(recs)]
    assert f["status"][small] == 6 and int(f["n_samples"][small]) == 4000 and not np.delete(f["status"], small).any()
    n, G = len(recs), 8
    out = torch.from_numpy(np.full(G + n + G, GUARD, dtype=np.uint64).view(np.int64)).to(dec.dev)
    st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
    gpu.lib.check(L.s5gpu_digest_dev(n, dec.t_desc.data_ptr(), dec.t_scr.data_ptr(), dec.t_sig.data_ptr(), dec.t_fields.data_ptr(), ob.SIG_EX_ZD,
                                     out.data_ptr() + 8 * G, st), "s5gpu_digest_dev")
    torch.cuda.synchronize(dec.dev)
    h = out.cpu().numpy().view(np.uint64)
    assert (h[:G] == GUARD).all() and (h[G + n:] == GUARD).all(), "guard words around the digests"
    want = crafted.ref[pick].copy()
    want[small] = 0
    assert np.array_equal(h[G:G + n], want)


@pytest.mark.gpu
def test_refused_arguments(gpu):
    L = gpu.L
    torch = gpu.torch
    rec = np.frombuffer(bytes(64), dtype=np.uint8)
    pos, ln = np.array([8], dtype=np.uint64), np.array([16], dtype=np.uint32)
    dig, st = np.full(1, 7, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    p = lambda a: a.ctypes.data
    assert L.s5gpu_digest_stream(0, None, 0, None, None, 1, 1, None, None) == 0                     # n == 0
    assert L.s5gpu_digest_batch(0, None, None, 1, 1, None, None) == 0
    assert L.s5gpu_digest_dev(0, None, None, None, None, 1, None, None) == 0
    assert L.s5gpu_digest_stream(1, p(rec), 64, p(pos), p(ln), 3, 1, p(dig), p(st)) == -1 and b"method" in L.s5gpu_last_error()
    assert L.s5gpu_digest_stream(1, p(rec), 64, p(pos), p(ln), 1, 3, p(dig), p(st)) == -1
    assert L.s5gpu_digest_batch(1, None, None, 1, -1, p(dig), p(st)) == -1
    assert L.s5gpu_digest_dev(1, None, None, None, None, 7, None, None) == -1
    assert L.s5gpu_digest_stream(1, None, 64, p(pos), p(ln), 1, 1, p(dig), p(st)) == -1 and b"NULL" in L.s5gpu_last_error()
    assert L.s5gpu_digest_stream(1, p(rec), 64, p(pos), p(ln), 1, 1, None, p(st)) == -1
    assert L.s5gpu_digest_batch(1, None, None, 1, 1, p(dig), p(st)) == -1
    far = np.array([60], dtype=np.uint64)
    assert L.s5gpu_digest_stream(1, p(rec), 64, p(far), p(ln), 1, 1, p(dig), p(st)) == -1 and b"outside" in L.s5gpu_last_error()
    d = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a = d.data_ptr()
    assert L.s5gpu_digest_dev(1, a, a, a, a, 1, None, None) == -1 and b"NULL" in L.s5gpu_last_error()
    assert L.s5gpu_digest_dev(1, a, a + 8, a, a, 1, a, None) == -1 and b"misaligned" in L.s5gpu_last_error()
    assert L.s5gpu_digest_dev(1, a, a, a + 2, a, 1, a, None) == -1
    assert L.s5gpu_digest_dev(1, a, a, a, a, 1, a + 4, None) == -1
    torch.cuda.synchronize()
    assert dig[0] == 7 and not d.cpu().numpy().any()                                                 # nothing was written


# ---------------------------------------------------------------------------------------------------------------- s5sum

def s5sum(*args, chunk_kb=None):
    env = dict(os.environ)
    env.pop("S5SUM_CHUNK_KB", None)
    if chunk_kb:
        env["S5SUM_CHUNK_KB"] = str(chunk_kb)
    return subprocess.run([S5SUM] + [str(a) for a in args], capture_output=True, env=env, timeout=120)


@pytest.mark.gpu
@pytest.mark.parametrize("rel", ALL)
def test_s5sum_on_every_golden_file(rel):
    p = s5sum(golden(rel))
    if rel == DUPLICATE:
        assert p.returncode == 2 and b"more than once" in p.stderr and p.stdout == b""
        return
    assert p.returncode == 0, p.stderr
    assert p.stdout == sum_lines(golden(rel))


def test_the_golden_set_holds_the_files_the_tool_must_cope_with():
    assert len(ALL) >= 40 and DUPLICATE in ALL
    for rel in ("ref/raw/degrade/p2solo_ulk114_dna.blow5", "aux_array_exp_lossless.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5",
                "exp_1_lossless_zlib_ex_zd.blow5", "ref/raw/skim/sequin_rna.blow5"):
        assert rel in ALL, rel
    f = Blow5(golden("ref/raw/degrade/p2solo_ulk114_dna.blow5"))
    assert len(f.records) == 1 and len(pieces(depress(f.records[0], f.rec_method), f.sig_method)[1]) == 2050027
    assert any(b"enum{" in Blow5(golden(r)).header_text for r in ALL)                                # the enum headers


@pytest.mark.gpu
@pytest.mark.parametrize("rel", ["example_multi_rg_v0.2.0.blow5", "example_multi_rg_v0.2.0_zstd_svb-zd.blow5", "example_multi_rg_v0.1.0.blow5",
                                 "merged_expected_zlib_svb.blow5"])
def test_s5sum_batch_and_chunk_sizes_give_the_same_bytes(rel):
    want = sum_lines(golden(rel))
    for args, kb in ((("-K", 1), None), (("-K", 3), None), (("-K", 4096), None), ((), 4), (("-K", 3), 4)):
        p = s5sum(*args, golden(rel), chunk_kb=kb)
        assert p.returncode == 0 and p.stdout == want, (args, kb, p.stderr)


@pytest.mark.gpu
def test_s5sum_reads_slow5_ascii_and_the_python_call_agrees(gpu):
    want = sum_lines(golden("exp_1_lossless.blow5")).split(b"\n")
    p = s5sum(golden("exp_1_lossless.slow5"))
    assert p.returncode == 0, p.stderr
    got = p.stdout.split(b"\n")
    assert got[1] == want[1] and got[1].startswith(b"4ae2fef7913faf61\t") and got[2] == want[2]
    text = open(golden("exp_1_lossless.slow5"), "rb").read()
    hdr = b"".join(l + b"\n" for l in text.split(b"\n") if l[:1] in (b"#", b"@") and not l.startswith((b"#slow5_version", b"#num_read_groups")))
    assert got[0] == b"#s5sum\t1\txxh64\t%016x" % xxh64_once(hdr)
    # several lines per call and one line per call, a chunk smaller than a line
    multi = s5sum("-K", 2, golden("example_multi_rg_v0.1.0.slow5"), chunk_kb=4)
    assert multi.returncode == 0, multi.stderr
    # (the reference is the TEXT's: a float aux field printed in decimal need not parse back to the bytes its BLOW5 twin holds)
    ids, digs = slow5_ref(golden("example_multi_rg_v0.1.0.slow5"))
    assert len(ids) == 7 and multi.stdout.split(b"\n")[1:] == [b"%016x\t%s" % (d, i) for i, d in zip(ids, digs)] + [b"#total\t7\t%016x" % (sum(digs) & (2 ** 64 - 1)), b""]
    ids, digs, hd = gpu.digest.file_digests(golden("example_multi_rg_v0.2.0.blow5"), batch=3)
    rids, rdigs, f = file_ref(golden("example_multi_rg_v0.2.0.blow5"))
    assert ids == rids and digs.tolist() == rdigs and hd == xxh64_once(f.header_text)


@pytest.mark.gpu
def test_s5sum_compare():
    one = "ref/exp/one_fast5/"
    for a, b in (("exp_1_lossless.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5"), ("exp_1_lossless_zlib_ex_zd.blow5", "exp_1_lossless.slow5"),
                 ("example_multi_rg_v0.1.0.blow5", "example_multi_rg_v0.2.0_zstd_svb-zd.blow5"), ("aux_array_exp_lossless.blow5", "exp_lossless_gzip.blow5"),
                 ("ref/exp/f2s/multi-fast5-output/ssm1_zlib.blow5", "ref/exp/f2s/multi-fast5-output/ssm1_zlib_svb.blow5")):
        p = s5sum("--compare", golden(a), golden(b))
        n = len(file_ref(golden(a))[0]) if a.endswith(".blow5") else 1
        lines = p.stdout.split(b"\n")
        assert p.returncode == 0 and lines[-2] == b"same\t%d" % n, (a, b, p.stdout, p.stderr)
        assert all(l.startswith(b"header\t") for l in lines[:-2])              # a header difference does not change the exit code
    p = s5sum("--compare", golden("exp_1_lossless.blow5"), golden(one + "exp_1_lossy.blow5"))
    lines = p.stdout.split(b"\n")
    rid = file_ref(golden("exp_1_lossless.blow5"))[0][0]
    assert p.returncode == 1 and lines[0].startswith(b"header\t") and lines[2:] == [b"same\t0", b""]
    assert lines[1] == b"differs\t%s\t4ae2fef7913faf61\tac1617e03ec409c2" % rid
    a, b = "example_multi_rg_v0.2.0.blow5", "ref/exp/get/expected_extracted_reads.blow5"
    p = s5sum("--compare", golden(a), golden(b))
    ia, ib = file_ref(golden(a))[0], file_ref(golden(b))[0]
    assert not set(ia) & set(ib)
    want = [(i, b"only-in-a\t" + i) for i in ia] + [(i, b"only-in-b\t" + i) for i in ib]
    lines = [l for l in p.stdout.split(b"\n") if not l.startswith(b"header\t")]
    assert p.returncode == 1 and lines == [l for _, l in sorted(want)] + [b"same\t0", b""]
    p = s5sum("--compare", golden(DUPLICATE), golden(DUPLICATE))
    assert p.returncode == 2 and b"more than once" in p.stderr
    assert s5sum("--compare", golden(a)).returncode == 2 and s5sum(golden("no_such_file.blow5")).returncode == 2
