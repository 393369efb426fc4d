"""stats: the s5stats tool and the file-wide signal accumulator made on the device (k_file_stats, docs/codecs.md §4.13).

The oracle is numpy over the int16 arrays a test made itself (or that oracle_bind decoded): bincount, sums in int64, bitwise_or.reduce.
Every statistic is an integer sum, min, max, OR or AND, so every comparison is exact.

  not gpu : s5stats against the reference's expected outputs (tests/golden/stats), its exit codes on the files the reference's own tests
            expect to fail, the layout of s5gpu_file_stats_t against the numpy dtype, the exports and bindings.
  gpu     : one batch of every length class and value kind through three decode forms; the window / bins / flush / grid options (fewer
            workgroups than records, so that flushes between records empty counters that hold samples); 3000 short reads; hand-made device
            buffers between guard words; accumulation over calls and past a corrupt record; degrade; every good reference file; the tool.

The batch holds -32768 and 32767 and the window has at most 2048 bins, so no window holds every sample of the whole batch: the run with every
sample inside the window takes the batch without the one read that holds the two extremes (asserted below); every other run takes all of it.
"""
import ctypes as C
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import GOLDEN, Blow5, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S5STATS = os.path.join(ROOT, "slow5tools_amd", "s5stats")
REF = os.path.join(GOLDEN, "ref")
MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))
GOOD = sorted(k for k, v in MANIFEST.items() if not v.get("negative"))
NAMES = ["s5gpu_file_stats_bytes", "s5gpu_file_stats_reset_dev", "s5gpu_file_stats_accum_dev", "s5gpu_file_stats_open", "s5gpu_file_stats_add_stream",
         "s5gpu_file_stats_close"]
GUARD = 0xA5A5A5A5A5A5A5A5


def s5stats(*args):
    return subprocess.run([S5STATS] + [str(a) for a in args], capture_output=True, timeout=120)


# ---------------------------------------------------------------------------------------------------------------- the oracle

def oracle(sigs, rgs, n_failed=0):
    """the accumulator of reads with samples sigs[i] (int16 arrays) and read groups rgs[i], and n_failed failed records"""
    from slow5tools_amd._lib import FILE_STATS

    o = np.zeros(1, dtype=FILE_STATS)[0]
    x = np.concatenate([np.asarray(s, dtype=np.int16) for s in sigs] + [np.zeros(0, np.int16)])
    lens = [len(s) for s in sigs]
    o["n_reads"], o["n_failed"], o["n_samples"] = len(sigs), n_failed, x.size
    o["sum"] = int(x.astype(np.int64).sum())
    o["sumsq"] = int((x.astype(np.int64) ** 2).sum()) & (2 ** 64 - 1)
    o["min"], o["max"] = (int(x.min()), int(x.max())) if x.size else (32767, -32768)
    o["or_bits"] = int(np.bitwise_or.reduce(x.view(np.uint16))) if x.size else 0
    o["and_bits"] = int(np.bitwise_and.reduce(x.view(np.uint16))) if x.size else 0xFFFF
    o["len_min"], o["len_max"] = (min(lens), max(lens)) if lens else (0xFFFFFFFF, 0)
    for n, g in zip(lens, rgs):
        o["len_hist"][int(n).bit_length()] += 1                  # 0 samples: class 0, else 1 + floor(log2 n)
        if g < 256:
            o["rg_reads"][g] += 1
            o["rg_samples"][g] += n
        else:
            o["rg_other"] += 1
    o["hist"][:] = np.bincount(x.astype(np.int32) + 32768, minlength=65536)
    return o


def assert_same(got, want, what=""):
    for name in want.dtype.names:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if not np.array_equal(g, w):
            at = np.nonzero(np.atleast_1d(g != w))[0][:8]
            raise AssertionError("%s: %s differs at %s: got %s, want %s" % (what, name, at.tolist(), np.atleast_1d(g)[at].tolist(), np.atleast_1d(w)[at].tolist()))


def depress(rec, rec_method):
    if rec_method == ob.REC_ZLIB:
        return zlib.decompress(rec)
    if rec_method == ob.REC_ZSTD:
        out = ob.zstd_decompress(rec) if ob.zstd_ref() else ob.zstd_restated_decompress(rec, 16 * len(rec) + (1 << 20))
        assert out is not None
        return out
    return bytes(rec)


# ---------------------------------------------------------------------------------------------------------------- the batch

LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4000, 70001]
GROUPS = [0, 1, 255, 256, 70000]
EXTREMES = 4            # the read (of 9 samples) that holds -32768 and 32767
INSIDE_LO, INSIDE_BINS = 32768 - 512, 2048      # values -512 .. 1535


class Batch:
    def __init__(self):
        rng = np.random.default_rng(1313)
        self.sigs, self.rgs, self.recs = [], [], []
        for k, n in enumerate(LENGTHS):
            x = np.clip(np.rint(520 + 90 * rng.standard_normal(n)), -400, 1400).astype(np.int16)
            if n == 9:
                x[2], x[7] = -32768, 32767
            if n == 64:
                x[:] = 0                                          # the all-zero read
            if n == 255:
                x[:] = 517                                        # the constant read
            if n == 256:
                x = (x // 8 * 8).astype(np.int16)                 # multiples of 8
            self.sigs.append(x)
            self.rgs.append(GROUPS[k % len(GROUPS)])
            r, keep = ob.make_rec(b"read-%04d" % k, self.rgs[-1], 8192.0, 23.0, 1467.61, 4000.0, x, bytes(range(k % 7)))
            self.recs.append((r, keep))
        assert LENGTHS[EXTREMES] == 9 and set(self.rgs) == set(GROUPS)
        self.want = oracle(self.sigs, self.rgs)

    def stored(self, rec_method, sig_method, which=None):
        idx = range(len(self.recs)) if which is None else which
        return [ob.rec_to_mem(self.recs[i][0], rec_method, sig_method)[8:] for i in idx]


@pytest.fixture(scope="module")
def batch():
    return Batch()


def test_the_batch_holds_what_the_kernel_can_get_wrong(batch):
    """asserted on the CPU, before any GPU test relies on it"""
    w = batch.want
    assert w["min"] == -32768 and w["max"] == 32767 and w["len_min"] == 0 and w["len_max"] == 70001
    assert w["len_hist"][0] == 1 and w["len_hist"][17] == 1 and w["rg_other"] == len([g for g in batch.rgs if g >= 256]) >= 2
    assert w["rg_reads"][255] >= 2 and w["or_bits"] == 0xFFFF and w["and_bits"] == 0
    assert not batch.sigs[LENGTHS.index(64)].any() and (batch.sigs[LENGTHS.index(256)] % 8 == 0).all()
    # the three windows of the route test: all inside (without the read of the extremes), all outside, and cut by both edges
    rest = np.concatenate([s for i, s in enumerate(batch.sigs) if i != EXTREMES]).astype(np.int32) + 32768
    assert ((rest >= INSIDE_LO) & (rest < INSIDE_LO + INSIDE_BINS)).all()
    allv = np.concatenate(batch.sigs).astype(np.int32) + 32768
    assert not ((allv >= 32768 + 20000) & (allv < 32768 + 20000 + 64)).any()
    cut_lo = 32768 + 517                                          # a value present in the data
    assert (allv == cut_lo).any() and (allv < cut_lo).any() and (allv >= cut_lo + 64).any() and ((allv > cut_lo) & (allv < cut_lo + 64)).any()


# ---------------------------------------------------------------------------------------------------------------- not gpu

STATS_FILES = [("exp_1_lossless.slow5", golden("exp_1_lossless.slow5")), ("exp_1_lossy.blow5", golden("ref/raw/stats/exp_1_lossy.blow5")),
               ("zlib_svb-zd_multi_rg_v0.2.0.blow5", golden("ref/raw/stats/zlib_svb-zd_multi_rg_v0.2.0.blow5")),
               ("zlib_svb-zd_multi_rg_v1.0.0.blow5", golden("ref/raw/stats/zlib_svb-zd_multi_rg_v1.0.0.blow5"))]


@pytest.mark.parametrize("name,path", STATS_FILES)
def test_s5stats_prints_the_reference_lines(name, path):
    """test/test_stats.sh testcases 3 - 6: the expected file from line 2 on; line 1 names the path as it was given"""
    want = open(golden("stats/" + name.rsplit(".", 1)[0] + ".stdout"), "rb").read().split(b"\n")
    for arg, cwd in ((path, None), (os.path.relpath(path, GOLDEN), GOLDEN)):
        p = subprocess.run([S5STATS, arg], capture_output=True, timeout=120, cwd=cwd)
        assert p.returncode == 0, p.stderr
        got = p.stdout.split(b"\n")
        assert got[0] == b"file path\t" + arg.encode()
        assert got[1:] == want[1:] and len(got) == 10 and got[-1] == b""


def test_s5stats_refuses_a_version_above_1_0_0():
    """test/test_stats.sh testcase 7"""
    p = s5stats(golden("ref/raw/stats/zlib_svb-zd_multi_rg_v1.1.0.blow5"))
    assert p.returncode == 1 and b"1.1.0" in p.stderr and b"number of records" not in p.stdout


@pytest.mark.parametrize("name,ok", [("exp_1_lossy_bad_eof.blow5", False), ("zlib_svb-zd_multi_rg_v0.2.0_bad_hdr_len.blow5", False),
                                     ("zlib_svb-zd_multi_rg_v0.2.0_trunc.blow5", False), ("exp_1_lossy_good.blow5", True),
                                     ("zlib_svb-zd_multi_rg_v0.2.0_good.blow5", True)])
def test_s5stats_on_the_quickcheck_files(name, ok):
    p = s5stats(golden("ref/raw/quickcheck/" + name))
    if ok:
        assert p.returncode == 0 and p.stdout.split(b"\n")[8].startswith(b"number of records\t"), p.stderr
    else:
        assert p.returncode == 1 and p.stderr.startswith(b"s5stats: ") and b"number of records" not in p.stdout


def test_s5stats_refuses_bad_arguments():
    assert s5stats().returncode == 1 and s5stats("--hist", "x", golden("exp_1_lossless.blow5")).returncode == 1
    assert s5stats(golden("no_such_file.blow5")).returncode == 1 and s5stats("-K", 0, "--signal", golden("exp_1_lossless.blow5")).returncode == 1


def test_the_numpy_dtype_is_the_c_struct(tmp_path):
    from slow5tools_amd import _lib

    names = [n for n in _lib.FILE_STATS.names]
    src = tmp_path / "fs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){printf("%zu", sizeof(s5gpu_file_stats_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_file_stats_t, %s));\n' % n for n in names) + 'printf("\\n");return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "fs")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "fs")], text=True).split()]
    assert got[0] == _lib.FILE_STATS.itemsize == 528720
    assert got[1:] == [_lib.FILE_STATS.fields[n][1] for n in names]
    assert _lib.lib().s5gpu_file_stats_bytes() == got[0]


def test_library_exports_and_binds_the_stats_calls():
    from slow5tools_amd import _lib, fstats

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in NAMES if s not in exported] and not [s for s in NAMES if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert len(L.s5gpu_file_stats_accum_dev.argtypes) == 7 and len(L.s5gpu_file_stats_add_stream.argtypes) == 9
    assert callable(fstats.file_stats) and callable(fstats.accumulate) and callable(fstats.accum_dev)
    assert os.access(S5STATS, os.X_OK)
    for key, bad in ((b"fstats_window_lo", 65536), (b"fstats_lds_bins", 100), (b"fstats_lds_bins", 4096), (b"fstats_flush_samples", 0), (b"fstats_grid", 0),
                     (b"fstats_grid", 1025)):
        assert L.s5gpu_set_option(key, bad) == -1
    for key, good in ((b"fstats_window_lo", -1), (b"fstats_lds_bins", 2048), (b"fstats_flush_samples", 0xFFFFFFFF), (b"fstats_grid", 1024)):
        assert L.s5gpu_set_option(key, good) == 0                 # (the defaults)


def test_the_oracle_on_a_hand_made_case():
    o = oracle([np.array([-1, 0, 8], np.int16), np.zeros(0, np.int16)], [3, 300], n_failed=2)
    assert (o["n_reads"], o["n_failed"], o["n_samples"], o["sum"], o["sumsq"], o["min"], o["max"]) == (2, 2, 3, 7, 65, -1, 8)
    assert (o["or_bits"], o["and_bits"], o["len_min"], o["len_max"], o["rg_other"]) == (0xFFFF, 0, 0, 3, 1)
    assert o["len_hist"][0] == 1 and o["len_hist"][2] == 1 and o["len_hist"].sum() == 2 and o["rg_reads"][3] == 1 and o["rg_samples"][3] == 3
    assert o["hist"][32767] == 1 and o["hist"][32768] == 1 and o["hist"][32776] == 1 and o["hist"].sum() == 3


# ---------------------------------------------------------------------------------------------------------------- gpu

@pytest.fixture(scope="module")
def gpu():
    import torch
    from slow5tools_amd import _lib, fstats, press

    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.fstats, env.press = torch, _lib, _lib.lib(), fstats, press
    return env


@pytest.fixture
def options(gpu):
    def set_(**kw):
        for k, v in kw.items():
            gpu.lib.check(gpu.L.s5gpu_set_option(("fstats_" + k).encode(), v), k)

    yield set_
    set_(window_lo=-1, lds_bins=2048, flush_samples=0xFFFFFFFF, grid=1024)


def through_handle(gpu, recs, rec_method, sig_method):
    return gpu.fstats.accumulate(recs, rec_method, sig_method).close()


def through_dev(gpu, recs, rec_method, sig_method, no_payload):
    dec = gpu.press.decode_to_device(recs, rec_method, sig_method, no_payload=no_payload)
    return gpu.fstats.to_numpy(gpu.fstats.accum_dev(dec, gpu.fstats.new_acc()))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["zlib+svb-zd no payload", "zlib+svb-zd full", "none/none", "zlib+svb-zd chunk call"])
def test_the_batch_through_every_decode_form(gpu, batch, form):
    if form == "none/none":
        got = through_handle(gpu, batch.stored(ob.REC_NONE, ob.SIG_NONE), ob.REC_NONE, ob.SIG_NONE)
    elif form == "zlib+svb-zd chunk call":
        got = through_handle(gpu, batch.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD), ob.REC_ZLIB, ob.SIG_SVB_ZD)
    else:
        got = through_dev(gpu, batch.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD), ob.REC_ZLIB, ob.SIG_SVB_ZD, no_payload=form.endswith("no payload"))
    assert_same(got, batch.want, form)


@pytest.mark.gpu
def test_every_route_gives_the_same_accumulator(gpu, batch, options):
    recs = batch.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD)
    dec = gpu.press.decode_to_device(recs, ob.REC_ZLIB, ob.SIG_SVB_ZD)
    run = lambda d: gpu.fstats.to_numpy(gpu.fstats.accum_dev(d, gpu.fstats.new_acc()))
    for what, kw in (("every sample outside the window", dict(window_lo=32768 + 20000, lds_bins=64)),
                     ("the window's edges cut the data", dict(window_lo=32768 + 517, lds_bins=64)),
                     ("no LDS bins", dict(lds_bins=0)),
                     ("a flush every 1000 samples", dict(flush_samples=1000)),
                     ("a flush every 1000 samples, cut window", dict(flush_samples=1000, window_lo=32768 + 517, lds_bins=64)),
                     ("the window asked past the last bin", dict(window_lo=65535, lds_bins=128)),
                     ("the defaults", dict()),
                     # fewer workgroups than records: a workgroup walks several records, so a flush between two of them empties counters that
                     # hold the earlier records' samples, and the length and read-group tables are used by more than one record
                     ("one workgroup walks the whole batch", dict(grid=1)),
                     ("one workgroup, a flush every 1000 samples", dict(grid=1, flush_samples=1000)),
                     ("one workgroup, a flush every 300 samples, cut window", dict(grid=1, flush_samples=300, window_lo=32768 + 517, lds_bins=64)),
                     ("two workgroups, a flush every 1000 samples, cut window", dict(grid=2, flush_samples=1000, window_lo=32768 + 517, lds_bins=64)),
                     ("three workgroups, a flush every 100 samples", dict(grid=3, flush_samples=100)),
                     ("three workgroups, no LDS bins", dict(grid=3, lds_bins=0)),
                     ("five workgroups, a flush every 5000 samples, window around 0", dict(grid=5, flush_samples=5000, window_lo=32768 - 32, lds_bins=128))):
        options(window_lo=-1, lds_bins=2048, flush_samples=0xFFFFFFFF, grid=1024)
        options(**kw)
        assert_same(run(dec), batch.want, what)
    # every sample inside the window: the batch without the read that holds -32768 and 32767 (see the module's docstring)
    rest = [i for i in range(len(LENGTHS)) if i != EXTREMES]
    dec = gpu.press.decode_to_device([recs[i] for i in rest], ob.REC_ZLIB, ob.SIG_SVB_ZD)
    want = oracle([batch.sigs[i] for i in rest], [batch.rgs[i] for i in rest])
    for kw in (dict(), dict(flush_samples=1000), dict(grid=1), dict(grid=2, flush_samples=1000)):
        options(window_lo=INSIDE_LO, lds_bins=INSIDE_BINS, flush_samples=0xFFFFFFFF, grid=1024)
        options(**kw)
        assert_same(run(dec), want, "every sample inside the window %r" % (kw,))


@pytest.mark.gpu
def test_many_short_reads_share_workgroups(gpu, options):
    """3000 reads of 0 .. 47 samples on hand-made device buffers: more records than a launch has workgroups (1024), so every workgroup walks
    two or three of them with its stride.  With a flush every 40 samples the windows that are flushed between two records hold samples."""
    torch, L, lib = gpu.torch, gpu.L, gpu.lib
    rng = np.random.default_rng(77)
    n = 3000
    lens = rng.integers(0, 48, size=n)
    lens[:5] = [0, 47, 8, 1, 40]
    caps = lens + rng.integers(0, 3, size=n)
    off = np.concatenate([[0], np.cumsum((caps + 15) // 8 * 8)]).astype(np.int64)
    sig = np.full(int(off[-1]) + 64, 0x7FFF, dtype=np.int16)
    fields = np.zeros(n, dtype=lib.REC_FIELDS)
    fields["n_samples"] = lens
    fields["read_group"] = rng.choice([0, 1, 2, 255, 256, 70000], size=n)
    fields["status"][::97] = 2
    sigs, rgs = [], []
    for i in range(n):
        if fields["status"][i] == 0:
            x = np.clip(np.rint(520 + 90 * rng.standard_normal(lens[i])), -400, 1400).astype(np.int16)
            sig[off[i]:off[i] + lens[i]] = x
            sigs.append(x)
            rgs.append(int(fields["read_group"][i]))
    want = oracle(sigs, rgs, n_failed=int((fields["status"] != 0).sum()))
    assert want["n_failed"] == 31 and want["len_hist"][0] > 0 and want["rg_other"] > 0
    dev = torch.device("cuda:0")
    t_sig = torch.from_numpy(sig).to(dev)
    t_off = torch.from_numpy(off[:-1].copy()).to(dev)
    t_cap = torch.from_numpy(caps.astype(np.uint32).view(np.int32)).to(dev)
    t_fields = torch.from_numpy(fields.view(np.uint8).copy()).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for what, kw in (("the defaults", dict()), ("a flush every 40 samples", dict(flush_samples=40)),
                     ("a flush every 40 samples, cut window", dict(flush_samples=40, window_lo=32768 + 517, lds_bins=64)),
                     ("seven workgroups, a flush every 1000 samples", dict(grid=7, flush_samples=1000))):
        options(window_lo=-1, lds_bins=2048, flush_samples=0xFFFFFFFF, grid=1024)
        options(**kw)
        acc = gpu.fstats.new_acc()
        lib.check(L.s5gpu_file_stats_accum_dev(n, t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), t_fields.data_ptr(), acc.data_ptr(), st), "accum")
        torch.cuda.synchronize(dev)
        assert_same(gpu.fstats.to_numpy(acc), want, what)


@pytest.mark.gpu
def test_accum_dev_owns_only_its_samples_and_its_accumulator(gpu):
    """hand-made device buffers: every gap between n_eff and the next slot holds 0x7FFF; a record with status 6 whose n_samples is larger than
    its slot, one with status 2, and one whose n_samples passes its slot with status 0 (n_eff is the slot's size)"""
    torch, L, lib = gpu.torch, gpu.L, gpu.lib
    rng = np.random.default_rng(5)
    #        n_samples, cap, status, read group
    plan = [(100, 100, 0, 0), (37, 64, 0, 1), (5000, 96, 6, 1), (0, 8, 0, 2), (300, 304, 2, 2), (9, 16, 0, 300), (70, 64, 0, 255), (1000, 1001, 0, 0)]
    n = len(plan)
    caps = np.array([p[1] for p in plan], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum((caps + 15) // 8 * 8)]).astype(np.int64)
    sig = np.full(int(off[-1]) + 64, 0x7FFF, dtype=np.int16)
    fields = np.zeros(n, dtype=lib.REC_FIELDS)
    sigs, rgs = [], []
    for i, (ns, cap, st, rg) in enumerate(plan):
        fields[i]["status"], fields[i]["n_samples"], fields[i]["read_group"] = st, ns, rg
        if st == 0:
            ne = min(ns, cap)
            x = rng.integers(200, 900, size=ne).astype(np.int16)
            x[::17] = 32767                                         # real samples of the guard's value
            sig[off[i]:off[i] + ne] = x
            sigs.append(x)
            rgs.append(rg)
    want = oracle(sigs, rgs, n_failed=2)
    dev = torch.device("cuda:0")
    G = 8
    t_sig = torch.from_numpy(sig).to(dev)
    t_off = torch.from_numpy(off[:-1].copy()).to(dev)
    t_cap = torch.from_numpy(caps.astype(np.uint32).view(np.int32)).to(dev)
    t_fields = torch.from_numpy(fields.view(np.uint8).copy()).to(dev)
    words = lib.FILE_STATS.itemsize // 8
    t_acc = torch.from_numpy(np.full(G + words + G, GUARD, dtype=np.uint64).view(np.int64)).to(dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    acc = t_acc.data_ptr() + 8 * G
    lib.check(L.s5gpu_file_stats_reset_dev(acc, st), "reset")
    lib.check(L.s5gpu_file_stats_accum_dev(n, t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), t_fields.data_ptr(), acc, st), "accum")
    torch.cuda.synchronize(dev)
    h = t_acc.cpu().numpy().view(np.uint64)
    assert (h[:G] == GUARD).all() and (h[G + words:] == GUARD).all(), "guard words around the accumulator"
    got = h[G:G + words].view(lib.FILE_STATS)[0]
    assert got["n_failed"] == 2 and got["hist"][65535] == sum(int((s == 32767).sum()) for s in sigs)
    assert_same(got, want, "hand-made buffers")
    assert (t_sig.cpu().numpy() == sig).all()                      # the input is read only
    # refused arguments: nothing is launched
    assert L.s5gpu_file_stats_accum_dev(n, t_sig.data_ptr() + 2, t_off.data_ptr(), t_cap.data_ptr(), t_fields.data_ptr(), acc, st) == -1
    assert L.s5gpu_file_stats_accum_dev(n, t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), t_fields.data_ptr(), acc + 4, st) == -1
    assert L.s5gpu_file_stats_accum_dev(n, None, t_off.data_ptr(), t_cap.data_ptr(), t_fields.data_ptr(), acc, st) == -1
    assert L.s5gpu_file_stats_reset_dev(None, st) == -1 and L.s5gpu_file_stats_accum_dev(0, None, None, None, None, acc, st) == 0


@pytest.mark.gpu
def test_accumulation_over_calls_and_past_a_corrupt_record(gpu, batch):
    recs = batch.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD)
    half = len(recs) // 2
    h = gpu.fstats.accumulate(recs[:half], ob.REC_ZLIB, ob.SIG_SVB_ZD)
    assert gpu.fstats.accumulate(recs[half:], ob.REC_ZLIB, ob.SIG_SVB_ZD, handle=h) is h
    assert_same(h.close(), batch.want, "two halves")
    # one flipped byte inside a zlib stream, beside a long constant read whose payload outgrows the slot the decoder guesses for it
    const = np.full(60000, 517, dtype=np.int16)
    r, keep = ob.make_rec(b"long-constant", 1, 8192.0, 23.0, 1467.61, 4000.0, const, b"")
    first = recs[half:] + [ob.rec_to_mem(r, ob.REC_ZLIB, ob.SIG_SVB_ZD)[8:]]
    bad = LENGTHS.index(4000)
    assert bad >= half
    flipped = bytearray(first[bad - half])
    flipped[len(flipped) // 2] ^= 0x5A
    first[bad - half] = bytes(flipped)
    h = gpu.fstats.Handle()
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        h.add(first, ob.REC_ZLIB, ob.SIG_SVB_ZD)
    st = h.add(recs[:half], ob.REC_ZLIB, ob.SIG_SVB_ZD)            # the handle still works
    assert not st.any()
    good = [i for i in range(len(recs)) if i != bad]
    want = oracle([batch.sigs[i] for i in good] + [const], [batch.rgs[i] for i in good] + [1], n_failed=1)
    assert_same(h.close(), want, "past a corrupt record")
    h = gpu.fstats.Handle()
    st = h.add(first, ob.REC_ZLIB, ob.SIG_SVB_ZD, raise_on_error=False)
    assert st[bad - half] != 0 and not np.delete(st, bad - half).any()
    h.abandon()
    # all nine press pairs through the chunk call on a few records
    pick = [LENGTHS.index(n) for n in (0, 9, 257, 4000)]
    want = oracle([batch.sigs[i] for i in pick], [batch.rgs[i] for i in pick])
    for rm in (ob.REC_NONE, ob.REC_ZLIB):
        for sm in (ob.SIG_NONE, ob.SIG_SVB_ZD, ob.SIG_EX_ZD):
            assert_same(through_handle(gpu, batch.stored(rm, sm, pick), rm, sm), want, (rm, sm))
    for sm in (ob.SIG_NONE, ob.SIG_SVB_ZD, ob.SIG_EX_ZD):
        frames = []
        for i in pick:
            pay = ob.rec_pack(batch.recs[i][0], sm)
            frames.append(ob.zstd_compress(pay) if ob.zstd_ref() else ob.zstd_literals_compress(pay))
        assert_same(through_handle(gpu, frames, ob.REC_ZSTD, sm), want, ("zstd", sm))


@pytest.mark.gpu
def test_a_degraded_batch_shows_its_constant_low_bits(gpu, batch):
    torch, L = gpu.torch, gpu.L
    recs = batch.stored(ob.REC_ZLIB, ob.SIG_SVB_ZD)
    dec = gpu.press.decode_to_device(recs, ob.REC_ZLIB, ob.SIG_SVB_ZD)
    t_off = torch.from_numpy(dec.sig_off.astype(np.int64)).to(dec.dev)
    t_n = torch.from_numpy(np.array(LENGTHS, dtype=np.uint32).view(np.int32)).to(dec.dev)
    st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
    gpu.lib.check(L.s5gpu_qts_round_dev(dec.t_sig.data_ptr(), len(recs), t_off.data_ptr(), t_n.data_ptr(), 3, st), "s5gpu_qts_round_dev")
    got = gpu.fstats.to_numpy(gpu.fstats.accum_dev(dec, gpu.fstats.new_acc()))

    def qts(x, bits=3):
        y = ((x.astype(np.int32) + (1 << (bits - 1))) >> bits) << bits
        return np.where(y > 32767, y - (1 << bits), y).astype(np.int16)

    want = oracle([qts(s) for s in batch.sigs], batch.rgs)
    assert got["or_bits"] & 7 == 0 and got["n_samples"] == batch.want["n_samples"]
    assert_same(got, want, "after qts rounding at 3 bits")


@pytest.mark.gpu
@pytest.mark.parametrize("rel", GOOD)
def test_every_good_reference_file(gpu, rel):
    """fstats.file_stats against the oracle over oracle_bind's decode of the same records (no file is skipped: the 2 050 027-sample record
    decodes in well under the time a test may take)"""
    m = MANIFEST[rel]
    f = Blow5(os.path.join(REF, rel))
    sigs, rgs = [], []
    for body in f.records:
        d = ob.rec_parse(depress(body, m["rec_method"]), m["sig_method"])
        sigs.append(d["signal"])
        rgs.append(d["read_group"])
    assert [len(s) for s in sigs] == [r["n_samples"] for r in m["records"]]
    assert_same(gpu.fstats.file_stats(os.path.join(REF, rel), batch=3), oracle(sigs, rgs), rel)


LOSSLESS = ["exp_1_lossless.blow5", "exp_1_lossless_v0.2.0.blow5", "exp_1_lossless_zlib.blow5", "exp_1_lossless_zlib_ex_zd.blow5",
            "exp_1_lossless_zlib_svb_v0.2.0.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5", "exp_1_lossless_zstd_v0.2.0.blow5"]


def signal_section(out):
    lines = out.split(b"\n")
    assert lines[8].startswith(b"number of records\t") and lines[9].startswith(b"total samples\t") and lines[-1] == b""
    return lines[9:-1]


@pytest.mark.gpu
def test_s5stats_signal_on_a_slow5_and_its_blow5_twins(gpu, tmp_path):
    p = s5stats("--signal", golden("exp_1_lossless.slow5"))
    assert p.returncode == 0, p.stderr
    plain = s5stats(golden("exp_1_lossless.slow5"))
    assert p.stdout.split(b"\n")[:9] == plain.stdout.split(b"\n")[:9]
    want = signal_section(p.stdout)
    f = Blow5(golden("exp_1_lossless.blow5"))
    sig = ob.rec_parse(f.records[0], ob.SIG_NONE)["signal"]
    srt = np.sort(sig)
    q = lambda x: int(srt[int(np.floor(x * (sig.size - 1)))])
    assert want[:12] == [b"total samples\t%d" % sig.size, b"sample min\t%d" % sig.min(), b"sample max\t%d" % sig.max(),
                         b"sample sum\t%d" % sig.astype(np.int64).sum(), b"sample sum of squares\t%d" % (sig.astype(np.int64) ** 2).sum(),
                         b"constant low bits\t0", b"sample median\t%d" % q(0.5), b"sample 1st percentile\t%d" % q(0.01),
                         b"sample 99th percentile\t%d" % q(0.99), b"sample mean\t%.3f" % (sig.astype(np.int64).sum() / sig.size),
                         b"read length min\t%d" % sig.size, b"read length max\t%d" % sig.size]
    assert want[12:] == [b"reads of length class %d\t1" % int(sig.size).bit_length(), b"read group 0\t1\t%d" % sig.size]
    for name in LOSSLESS:
        p = s5stats("--signal", golden(name))
        assert p.returncode == 0 and signal_section(p.stdout) == want, (name, p.stderr)
    # a file that says it was degraded: the lossy fixtures of degrade carry their bits in the name
    p = s5stats("--signal", golden("gridr10dna_b3.blow5"))
    assert p.returncode == 0 and b"constant low bits\t3" in p.stdout.split(b"\n"), p.stderr


@pytest.mark.gpu
def test_s5stats_batch_sizes_and_the_histogram_file(gpu, tmp_path):
    path = golden("example_multi_rg_v0.2.0.blow5")
    a, b = s5stats("--signal", "-K", 2, path), s5stats("--signal", "-K", 4096, "--hist", tmp_path / "h.tsv", path)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout, (a.stderr, b.stderr)
    sec = signal_section(a.stdout)
    total = int(sec[0].split(b"\t")[1])
    f = Blow5(path)
    sigs = [ob.rec_parse(depress(r, f.rec_method), f.sig_method) for r in f.records]
    assert total == sum(d["signal"].size for d in sigs)
    rows = [l.split("\t") for l in open(tmp_path / "h.tsv").read().split("\n") if l]
    vals = [int(r[0]) for r in rows]
    assert vals == sorted(set(vals)) and all(int(r[1]) > 0 for r in rows) and sum(int(r[1]) for r in rows) == total
    want = np.bincount(np.concatenate([d["signal"] for d in sigs]).astype(np.int32) + 32768, minlength=65536)
    assert vals == (np.nonzero(want)[0] - 32768).tolist() and [int(r[1]) for r in rows] == want[want > 0].tolist()
    groups = [l for l in sec if l.startswith(b"read group ")]
    assert len(groups) == f.num_read_groups
    for g, l in enumerate(groups):
        assert l == b"read group %d\t%d\t%d" % (g, sum(d["read_group"] == g for d in sigs), sum(d["signal"].size for d in sigs if d["read_group"] == g))
    # a corrupt record: exit 1 and nothing of the signal section
    raw = bytearray(f.raw)
    raw[f.offsets[2] + 8 + len(f.records[2]) // 2] ^= 0x5A
    (tmp_path / "bad.blow5").write_bytes(bytes(raw))
    p = s5stats("--signal", tmp_path / "bad.blow5")
    assert p.returncode == 1 and b"total samples" not in p.stdout and b"corrupt" in p.stderr
