"""slow5tools degrade (src/degrade.c): qts rounding of every sample, then the view worker's re-encode (zlib + ex-zd by default,
src/degrade.c:302).  The rule (include/slow5gpu.h, s5gpu_qts_round_dev):

    y = ((x + 2^(b-1)) >> b) << b   in int32, arithmetic shift;   y > 32767: y -= 2^b

  not gpu : qts_ref against the reference's 8 raw / degraded pairs (tests/golden/ref/{raw,exp}/degrade): the signals, and the whole
            record rebuilt by the oracle; qts_ref on hand-made edge cases; the library exports every new symbol.
  gpu     : k_qts_round through s5gpu_qts_round_dev (every b, awkward lengths, guard patterns), the _qts batch call for every output
            press, s5view --degrade against the reference's files in every pipeline, the ASCII sides, refused bits.
"""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import GOLDEN, Blow5, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S5VIEW = os.path.join(ROOT, "slow5tools_amd", "s5view")
LIB = os.path.join(ROOT, "slow5tools_amd", "libslow5gpu.so")
RAW = os.path.join(GOLDEN, "ref", "raw", "degrade")
EXP = os.path.join(GOLDEN, "ref", "exp", "degrade")
PAIRS = sorted((f, g) for f in os.listdir(RAW) if f.endswith(".blow5")
               for g in os.listdir(EXP) if g.startswith(f[: -len(".blow5")] + "_b"))
assert len(PAIRS) == 8


def bits_of(exp_name):
    return int(re.search(r"_b(\d+)\.blow5$", exp_name).group(1))


def qts_ref(x, b):
    """the rule in numpy (int32 arithmetic; >> on numpy ints is arithmetic)"""
    x = np.asarray(x, dtype=np.int16).astype(np.int32)
    y = ((x + (1 << (b - 1))) >> b) << b
    y = np.where(y > 32767, y - (1 << b), y)
    return y.astype(np.int16)


def _unwrap(body, rec_method):
    if rec_method == ob.REC_ZLIB:
        return zlib.decompress(body)
    if rec_method == ob.REC_ZSTD:
        return ob.zstd_decompress(body)
    return body


def _parse(body, rec_method, sig_method):
    return ob.rec_parse(_unwrap(body, rec_method), sig_method)


def _rebuild(g, signal, rec_method, sig_method, pack=False):
    r, keep = ob.make_rec(g["read_id"], g["read_group"], g["digitisation"], g["offset"], g["range"], g["sampling_rate"], signal, g["aux"])
    return ob.rec_pack(r, sig_method) if pack else ob.rec_to_mem(r, rec_method, sig_method)


# ---------------------------------------------------------------------------------------------------------------- not gpu

@pytest.mark.parametrize("raw,exp", PAIRS)
def test_qts_ref_rebuilds_the_reference_degraded_records(raw, exp):
    """every read of the pair: qts_ref(raw, b) is the expected signal, and the oracle's record of it is the expected record, byte for byte"""
    b = bits_of(exp)
    src, dst = Blow5(os.path.join(RAW, raw)), Blow5(os.path.join(EXP, exp))
    assert len(src.records) == len(dst.records) and dst.rec_method == ob.REC_ZLIB
    for rs, rd in zip(src.records, dst.records):
        g = _parse(rs, src.rec_method, src.sig_method)
        e = _parse(rd, dst.rec_method, dst.sig_method)
        got = qts_ref(g["signal"], b)
        assert np.array_equal(got, e["signal"]), g["read_id"]
        mem = _rebuild(g, got, ob.REC_ZLIB, dst.sig_method)
        assert mem == struct.pack("<Q", len(rd)) + rd, g["read_id"]


def test_qts_ref_edge_cases():
    rng = np.random.default_rng(5)
    rnd = rng.integers(-32768, 32768, size=4096).astype(np.int16)
    for b in range(1, 17):
        s, h = 1 << b, 1 << (b - 1)
        if b <= 13:                                                   # ties either side of zero go toward +inf
            assert qts_ref([h, -h, 3 * h, -3 * h, h - 1, -h - 1], b).tolist() == [s, 0, 2 * s, -s, 0, -s], b
        assert qts_ref([-32768], b)[0] == (-32768 if b < 16 else 0)   # a multiple of 2^b (b <= 15); b = 16: the tie rounds up to 0
        assert qts_ref([32767], b)[0] == (32768 - s if b < 16 else 0)   # 32767 rounds to 32768 and steps down by 2^b to stay an int16
        assert qts_ref([0, 1, -1], b).tolist() == ([0, 2, 0] if b == 1 else [0, 0, 0])
        y = qts_ref(rnd, b).astype(np.int32)
        assert np.all(y % s == 0) and np.all(np.abs(y - rnd.astype(np.int32)) <= s), b
    assert qts_ref([-6, -2, 2, 6], 2).tolist() == [-4, 0, 4, 8]
    assert qts_ref([32767, 32766, 32765], 1).tolist() == [32766, 32766, 32766]
    assert np.all(qts_ref(np.arange(-32768, 32768), 16) == 0)


def test_library_exports_the_degrade_symbols():
    from slow5tools_amd import build

    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    need = ["s5gpu_qts_round_dev", "s5gpu_recompress_batch_qts", "s5gpu_recompress_stream_qts", "s5gpu_ascii_to_blow5_batch_qts",
            "s5gpu_ascii_to_blow5_stream_qts", "s5gpu_blow5_to_ascii_batch_qts", "s5gpu_blow5_to_ascii_stream_qts",
            "slow5_gpu_convert_batch_qts", "slow5_rec_qts_round", "slow5_gpu_hook_convert_qts"]
    assert not [n for n in need if n not in names]


# ---------------------------------------------------------------------------------------------------------------- gpu

@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 4000, 100_000, 2_050_027]


@pytest.mark.gpu
def test_qts_round_dev_every_bits_awkward_lengths_guards_untouched(press):
    import torch
    from slow5tools_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(0x9D)
    offs, pos = [], 8
    for i, n in enumerate(LENGTHS):
        offs.append(pos)
        pos += (n + 7) // 8 * 8 + 8 * (1 + i % 3)                      # gaps of 8..24 samples (more where n is not a multiple of 8)
    total = pos + 16
    base = np.full(total, 0x2AAB, dtype=np.int16)                      # guard: odd, so any rounding would change it
    for o, n in zip(offs, LENGTHS):
        x = rng.integers(-32768, 32768, size=n, dtype=np.int32).astype(np.int16)
        if n >= 64:   # adversarial: ties of every b either side of zero, the extremes
            ties = np.array([(1 << (b - 1)) * k for b in range(1, 17) for k in (1, -1, 3, -3)], dtype=np.int64)
            ties = ((ties + 32768) % 65536 - 32768).astype(np.int16)
            sp = np.concatenate([ties, np.array([32767, -32767, -32768, 0, 1, -1], dtype=np.int16)])
            x[: min(n, len(sp))] = sp[: min(n, len(sp))]
        base[o:o + n] = x
    mask = np.ones(total, dtype=bool)
    for o, n in zip(offs, LENGTHS):
        mask[o:o + n] = False
    st = torch.cuda.current_stream().cuda_stream
    d_off = torch.tensor(np.array(offs, dtype=np.uint64).view(np.int64), device="cuda")
    d_len = torch.tensor(np.array(LENGTHS, dtype=np.uint32).view(np.int32), device="cuda")
    for b in range(1, 17):
        d_sig = torch.from_numpy(base.copy()).to("cuda")
        _lib.check(L.s5gpu_qts_round_dev(d_sig.data_ptr(), len(LENGTHS), d_off.data_ptr(), d_len.data_ptr(), b, st), "s5gpu_qts_round_dev")
        torch.cuda.synchronize()
        got = d_sig.cpu().numpy()
        assert np.array_equal(got[mask], base[mask]), b                 # guards around every record and in the gaps
        for o, n in zip(offs, LENGTHS):
            assert np.array_equal(got[o:o + n], qts_ref(base[o:o + n], b)), (b, n)
    d_sig = torch.from_numpy(base.copy()).to("cuda")
    for b in (0, 17):
        assert L.s5gpu_qts_round_dev(d_sig.data_ptr(), len(LENGTHS), d_off.data_ptr(), d_len.data_ptr(), b, st) == -1   # S5GPU_ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(d_sig.cpu().numpy(), base)


def _synth_records(n_reads=6):
    reads = []
    for i, n in enumerate([0, 1, 9, 4000, 20_001, 65][:n_reads]):
        sig = ob.synth_read(0xDE6 + i, i, n) if n else np.zeros(0, dtype=np.int16)
        sig = np.asarray(sig, dtype=np.int16).copy()
        if n > 20:
            sig[:8] = [-6, -2, 2, 6, 32767, -32768, -32767, 1]
        g = dict(read_id=ob.synth_read_id(i), read_group=i % 2, digitisation=8192.0, offset=23.0, range=1467.61, sampling_rate=4000.0,
                 aux=b"")
        reads.append((g, sig))
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("to_rec", [ob.REC_NONE, ob.REC_ZLIB, ob.REC_ZSTD])
@pytest.mark.parametrize("to_sig", [ob.SIG_NONE, ob.SIG_SVB_ZD, ob.SIG_EX_ZD])
def test_degrade_records_every_output_press(press, to_rec, to_sig):
    reads = _synth_records()
    src = [_rebuild(g, s, ob.REC_ZLIB, ob.SIG_SVB_ZD)[8:] for g, s in reads]         # (without the u64 size)
    for b in (1, 3, 8, 16):
        out = press.degrade_records(src, b, ob.REC_ZLIB, ob.SIG_SVB_ZD, to_rec, to_sig)
        for (g, s), rec in zip(reads, out):
            body = rec[8:]
            assert struct.unpack_from("<Q", rec, 0)[0] == len(body)
            want = _rebuild(g, qts_ref(s, b), to_rec, to_sig, pack=True)
            got = _unwrap(body, to_rec)
            assert got == want, (b, g["read_id"])
            if to_sig == ob.SIG_EX_ZD and np.any(qts_ref(s, b)):       # (an all-zero signal gets q = 0: oracle/exzd.c)
                assert _exzd_q(got) >= b, (b, g["read_id"])


def _exzd_q(payload):
    """the q byte of the ex-zd blob in a record payload (oracle/rec.c, oracle/exzd.c): u16 id_len | id | u32 rg | 4 f64 | u64 L |
    blob = u8 version | u64 N | u8 q | ..."""
    idl = struct.unpack_from("<H", payload, 0)[0]
    return payload[2 + idl + 4 + 32 + 8 + 9]


def _run(args, env=None, check=True):
    r = subprocess.run([S5VIEW] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def _press_args(raw):
    return ["zlib", "svb-zd"] if raw.startswith("promr10dna4khz") else ["zlib", "ex-zd"]


MODES = {
    "chunked": ({}, "4096", "2"),
    "per_record": ({"S5VIEW_PER_RECORD": "1"}, "3", "2"),
    "serial": ({}, "3", "0"),
    "three_devices": ({"S5GPU_ALIAS_DEVICES": "1", "S5VIEW_DEV_MASK": "7", "S5GPU_MULTI_MIN": "8", "S5VIEW_CHUNK_KB": "256"}, "2", "2"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_s5view_degrade_reproduces_the_reference_files(tmp_path, mode):
    extra, K, workers = MODES[mode]
    env = dict(os.environ, **extra)
    for raw, exp in PAIRS:
        b = bits_of(exp)
        out = tmp_path / ("%s_%s" % (mode, exp))
        _run(["--degrade", b, os.path.join(RAW, raw), out] + _press_args(raw) + [K, workers], env=env)
        mine, ref = out.read_bytes(), open(os.path.join(EXP, exp), "rb").read()
        m, r = Blow5(str(out)), Blow5(os.path.join(EXP, exp))
        assert mine[:68] == ref[:68] and m.header_text == r.header_text and mine[-5:] == ref[-5:] == b"5WOLB", exp
        assert len(m.records) == len(r.records), exp
        for a, e in zip(m.records, r.records):
            assert zlib.decompress(a) == zlib.decompress(e), exp
        assert len(mine) <= 1.02 * len(ref), (exp, len(mine), len(ref))


def _slow5_signals(path):
    return [np.array(l.split("\t")[7].split(","), dtype=np.int64) for l in open(path) if l and l[0] not in "#@" and l.strip()]


@pytest.mark.gpu
@pytest.mark.parametrize("workers", ["2", "0"])
def test_degrade_ascii_sides(tmp_path, workers):
    b = 3
    slow5_in, blow5_in = golden("exp_1_lossless.slow5"), golden("exp_1_lossless_zlib_svb_v0.2.0.blow5")
    a, c = tmp_path / "from_text.blow5", tmp_path / "from_blow5.blow5"
    _run(["--degrade", b, slow5_in, a, "zlib", "ex-zd", "64", workers])
    _run(["--degrade", b, blow5_in, c, "zlib", "ex-zd", "64", workers])
    ma, mc = Blow5(str(a)), Blow5(str(c))
    assert len(ma.records) == len(mc.records) > 0
    assert [zlib.decompress(x) for x in ma.records] == [zlib.decompress(x) for x in mc.records]
    # BLOW5 -> .slow5 degraded == degraded to BLOW5, then viewed to .slow5
    t1, t2 = tmp_path / "direct.slow5", tmp_path / "viewed.slow5"
    _run(["--degrade", b, blow5_in, t1, "zlib", "svb-zd", "64", workers])
    _run([c, t2, "zlib", "svb-zd", "64", workers])
    assert t1.read_text() == t2.read_text()
    # SLOW5 -> SLOW5: the sample columns are qts_ref of the input's
    t3 = tmp_path / "text.slow5"
    _run(["--degrade", b, slow5_in, t3, "zlib", "svb-zd", "64", workers])
    got, src = _slow5_signals(t3), _slow5_signals(slow5_in)
    assert len(got) == len(src) > 0
    for g, s in zip(got, src):
        assert np.array_equal(g, qts_ref(s.astype(np.int16), b).astype(np.int64))


@pytest.mark.gpu
def test_bits_outside_1_to_16_are_refused(press, tmp_path):
    from slow5tools_amd import _lib

    L = _lib.lib()
    reads = _synth_records(4)
    src = [_rebuild(g, s, ob.REC_ZLIB, ob.SIG_SVB_ZD)[8:] for g, s in reads]
    n = len(src)
    vp = C.c_void_p
    bufs = [C.create_string_buffer(r, max(len(r), 1)) for r in src]
    rec_p = (vp * n)(*[C.addressof(x) for x in bufs])
    rl = (C.c_size_t * n)(*[len(r) for r in src])
    for b in (0, 17):
        out, out_len = (vp * n)(), (C.c_size_t * n)()
        assert L.s5gpu_recompress_batch_qts(n, rec_p, rl, 1, 1, 1, 2, None, 0, out, out_len, None, b) == -1
        assert L.s5gpu_blow5_to_ascii_batch_qts(n, rec_p, rl, 1, 1, 0, None, None, 0, out, out_len, None, b) == -1
        r = _run(["--degrade", b, golden("exp_1_lossless_zlib_svb_v0.2.0.blow5"), tmp_path / "x.blow5"], check=False)
        assert r.returncode != 0 and "usage" in r.stderr
    r = _run(["--degrade", "auto", golden("exp_1_lossless_zlib_svb_v0.2.0.blow5"), tmp_path / "y.blow5"], check=False)
    assert r.returncode != 0 and "usage" in r.stderr
