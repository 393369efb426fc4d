"""signals: per-read order statistics (k_sig_stats) and normalised windows (k_sig_windows) of decoded reads on the device.

The oracle is the numpy restatement in this file (stats_ref / norm_ref): every statistic is an integer, so the comparison is exact.

  not gpu : exported symbols, the s5gpu_sig_stats_t layout against the numpy dtype, chunk_plan's rule, the restatement against np.median.
  gpu     : exact statistics over a batch that mixes lengths and contents; failed records (status 6, corrupt) between guard words; windows
            in every mode and dtype; read_signals on golden files of four codec pairs; the chunk call; refused arguments.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import Blow5, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTILES = (0.0, 0.2, 0.9, 1.0)
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4000, 4097, 70001]
GUARD = 0x2AAB


# ---------------------------------------------------------------------------------------------------------------- the oracle

def stats_ref(x, quantiles=QUANTILES):
    """s5gpu_sig_stats_t of one read in numpy / Python integers"""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    n = len(x)
    r = dict(n=n, sum=0, sumsq=0, med2=0, mad4=0, min=0, max=0, q=[0, 0, 0, 0])
    if n == 0:
        return r
    s = np.sort(x)
    med2 = int(s[(n - 1) // 2] + s[n // 2])
    ks = np.sort(np.abs(2 * x - med2))
    r.update(sum=int(x.sum()), sumsq=int((x * x).sum()), med2=med2, mad4=int(ks[(n - 1) // 2] + ks[n // 2]), min=int(s[0]), max=int(s[-1]))
    for k, q in enumerate(quantiles):
        r["q"][k] = int(s[int(np.floor(np.float64(q) * np.float64(n - 1)))])
    return r


def norm_ref(x, mode, f, st, a=0.51, b=0.53):
    """the four normalisations in float64 (RAW and PA are then exact in float32; MEDMAD and QUANT are the float64 restatement)"""
    x = np.asarray(x, dtype=np.int16).astype(np.float64)
    if mode == "raw":
        return x
    if mode == "pa":
        return (x + np.float64(f["offset"])) * (np.float64(f["range"]) / np.float64(f["digitisation"]))
    if mode == "medmad":
        return (2.0 * x - st["med2"]) / (0.7413 * st["mad4"] if st["mad4"] else 1.0)
    q0, q1 = int(st["q"][0]), int(st["q"][1])                              # (Python integers: the int16 members would wrap in q0 + q1)
    return (x - a * (q0 + q1)) / max(b * (q1 - q0), 1.0)


def assert_stats_equal(got, want, what):
    for k in ("n", "sum", "sumsq", "med2", "mad4", "min", "max"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    assert [int(v) for v in got["q"]] == want["q"], (what, "q", got["q"], want["q"])
    assert int(got["reserved"]) == 0


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_the_signal_calls():
    from slow5tools_amd import _lib

    names = ["s5gpu_signal_stats_dev", "s5gpu_signal_windows_dev", "s5gpu_signal_stats_stream"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in names if s not in exported]
    assert not [s for s in names if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert len(L.s5gpu_signal_stats_dev.argtypes) == 9 and len(L.s5gpu_signal_windows_dev.argtypes) == 17 and len(L.s5gpu_signal_stats_stream.argtypes) == 11


def test_sig_stats_layout_matches_header(tmp_path):
    from slow5tools_amd import signals

    members = ["n", "status", "sum", "sumsq", "med2", "mad4", "min", "max", "q", "reserved"]
    src = tmp_path / "ly.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){printf("%zu", sizeof(s5gpu_sig_stats_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_sig_stats_t, %s));\n' % m for m in members) + 'printf("\\n");return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "ly")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ly")], text=True).split()]
    D = signals.SIG_STATS
    assert got == [D.itemsize] + [D.fields[m][1] for m in members]
    assert D.itemsize == 48 and D["q"].shape == (4,)


@pytest.mark.parametrize("W,ov", [(64, 0), (64, 8), (4000, 0), (4000, 500)])
def test_chunk_plan_covers_every_sample(W, ov):
    from slow5tools_amd.signals import chunk_plan

    Ts = [0, 1, W - 1, W, W + 1, 2 * W - ov, 2 * W - ov + 1, 10 * W + 3]
    wr, ws = chunk_plan(Ts, W, ov)
    assert wr.dtype == np.uint32 and ws.dtype == np.uint32 and len(wr) == len(ws)
    assert (np.diff(wr.astype(np.int64)) >= 0).all()                     # the reads in order
    step = W - ov
    for i, T in enumerate(Ts):
        s = ws[wr == i].astype(np.int64)
        if T == 0:
            assert len(s) == 0
            continue
        if T <= W:
            assert s.tolist() == [0]
            continue
        k = (T - W) // step + 1
        want = [j * step for j in range(k)] + ([T - W] if (k - 1) * step + W != T else [])
        assert s.tolist() == want, (T, s)
        assert len(s) == k + ((k - 1) * step + W != T)                   # the count
        cover = np.zeros(T, dtype=bool)
        for b in s:
            assert b + W <= T                                            # no window passes T
            cover[b:b + W] = True
        assert cover.all() and s[-1] + W == T                            # every sample covered, the last window ends at T
    assert chunk_plan([], W, ov)[0].size == 0
    with pytest.raises(ValueError):
        chunk_plan([10], W, W)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000, 1001])
def test_restatement_is_numpy_median_and_mad(n):
    rng = np.random.default_rng(n)
    for hi in (32768, 40):                                               # wide, and narrow with many ties
        x = rng.integers(-hi, hi, size=n, dtype=np.int32).astype(np.int16)
        r = stats_ref(x)
        med = np.median(x.astype(np.float64))
        assert r["med2"] == 2 * med
        assert r["mad4"] == 4 * np.median(np.abs(x.astype(np.float64) - med))
        assert r["q"][0] == x.min() and r["q"][3] == x.max()
        assert r["q"][1] == np.quantile(x, 0.2, method="lower") and r["q"][2] == np.quantile(x, 0.9, method="lower")


# ---------------------------------------------------------------------------------------------------------------- gpu

def _contents(n, kind, rng):
    if kind == "synth":
        return ob.synth_reads(0x5105, n % 97, 1, n)[0] if n else np.zeros(0, np.int16)
    if kind == "constant":
        return np.full(n, 517, dtype=np.int16)
    if kind == "extremes":                                               # median 32767 for odd n: the MAD keys take all 17 bits
        return np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
    if kind == "two_valued":                                             # ties at the median
        return np.where(np.arange(n) % 3 == 0, -5, 9).astype(np.int16)
    if kind == "ramp":
        return (np.arange(n, dtype=np.int64) % 65536 - 32768).astype(np.int16)
    return rng.integers(-32768, 32768, size=n, dtype=np.int32).astype(np.int16)


KINDS = ["synth", "constant", "extremes", "two_valued", "ramp", "random"]


class Batch:
    """reads laid out as the decoder would leave them, with guard words between the slots"""

    def __init__(self, reads, caps, fields):
        self.reads, self.n = reads, len(reads)
        self.cap = np.asarray(caps, dtype=np.uint32)
        self.fields = fields
        pos, offs = 16, []
        for i, c in enumerate(self.cap):
            offs.append(pos)
            pos += (int(c) + 7) // 8 * 8 + 8 * (1 + i % 3)
        self.off = np.asarray(offs, dtype=np.uint64)
        self.base = np.full(pos + 16, GUARD, dtype=np.int16)
        self.mask = np.ones(pos + 16, dtype=bool)                          # True: a guard word
        for o, c, x in zip(offs, self.cap, reads):
            self.base[o:o + int(c)] = -1234                                # slot space behind the samples
            m = min(len(x), int(c))
            self.base[o:o + m] = x[:m]
            self.mask[o:o + int(c)] = False


def _golden_fields():
    f = Blow5(golden("exp_1_lossless.blow5"))
    g = ob.rec_parse(f.records[0], ob.SIG_NONE)
    assert g["digitisation"] == 8192.0 and abs(g["range"] - 1467.61) < 1e-2
    return g


@pytest.fixture(scope="module")
def gpu():
    """the library initialised, the mixed batch, and its statistics made ONCE on the device (shared by the tests; left unchanged)"""
    import torch
    from slow5tools_amd import _lib, press, signals

    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    rng = np.random.default_rng(7)
    reads = [_contents(n, KINDS[(i + j) % len(KINDS)], rng) for j in range(len(KINDS)) for i, n in enumerate(LENGTHS)]   # short and long in turn
    g = _golden_fields()
    fields = np.zeros(len(reads), dtype=_lib.REC_FIELDS)
    fields["n_samples"] = [len(x) for x in reads]
    for i in range(len(reads)):
        if i % 2 == 0:
            fields["digitisation"][i], fields["offset"][i], fields["range"][i] = g["digitisation"], g["offset"], g["range"]
        else:
            fields["digitisation"][i], fields["offset"][i], fields["range"][i] = 2048.0, -243.0, 748.5801
    fields["sampling_rate"] = 4000.0
    caps = [len(x) + (5 if i % 2 else 0) for i, x in enumerate(reads)]     # a slot may be longer than its read
    b = Batch(reads, caps, fields)
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.press, env.signals, env.batch = torch, _lib, _lib.lib(), press, signals, b
    env.ref = [stats_ref(x) for x in reads]
    return env


def _run_stats(env, b, quantiles=QUANTILES):
    """k_sig_stats over a Batch -> (stats, the stats buffer's guard bytes intact?, the device tensors for a window call)"""
    torch, L, S = env.torch, env.L, env.signals
    d_sig = torch.from_numpy(b.base.copy()).to("cuda")
    d_off = torch.from_numpy(b.off.view(np.int64).copy()).to("cuda")
    d_cap = torch.from_numpy(b.cap.view(np.int32).copy()).to("cuda")
    d_f = torch.from_numpy(b.fields.view(np.uint8).copy()).to("cuda")
    pad = 2 * S.SIG_STATS.itemsize
    d_st = torch.full((pad + b.n * S.SIG_STATS.itemsize + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    q = (C.c_double * 4)(*quantiles)
    env.lib.check(L.s5gpu_signal_stats_dev(b.n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), len(quantiles), q,
                                           d_st.data_ptr() + pad, None), "s5gpu_signal_stats_dev")
    torch.cuda.synchronize()
    raw = d_st.cpu().numpy()
    assert (raw[:pad] == 0xA5).all() and (raw[len(raw) - pad:] == 0xA5).all(), "guard bytes around stats"
    got_sig = d_sig.cpu().numpy()
    assert np.array_equal(got_sig, b.base), "k_sig_stats wrote to the signals"
    stats = raw[pad:len(raw) - pad].view(S.SIG_STATS).copy()
    return stats, (d_sig, d_off, d_cap, d_f, d_st, pad)


@pytest.fixture(scope="module")
def gpu_stats(gpu):
    return _run_stats(gpu, gpu.batch)


@pytest.mark.gpu
def test_stats_are_exact_over_a_mixed_batch(gpu, gpu_stats):
    stats, _ = gpu_stats
    for i, want in enumerate(gpu.ref):
        assert int(stats["status"][i]) == 0
        assert_stats_equal(stats[i], want, (i, want["n"]))


@pytest.mark.gpu
def test_stats_with_fewer_quantiles_leave_the_rest_zero(gpu):
    b = gpu.batch
    small = Batch(b.reads[:20], b.cap[:20], b.fields[:20].copy())
    stats, _ = _run_stats(gpu, small, quantiles=(0.5,))
    for i, x in enumerate(small.reads):
        want = stats_ref(x, (0.5,))
        assert_stats_equal(stats[i], want, i)


@pytest.mark.gpu
def test_failed_records_are_not_read_and_carry_their_status(gpu):
    """a real decode: one record into a signal slot that is too small (status 6, n_samples = the count it needed) and one corrupt record;
    the statistics kernel then runs over the decoder's slots rebuilt between guard words"""
    press, signals = gpu.press, gpu.signals
    sig = ob.synth_reads(0x5105, 0, 5, 4000)
    hdrs = [press.pack_hdr(ob.synth_read_id(i), 0, 8192.0, 23.0, 1467.61, 4000.0) for i in range(5)]
    recs = [r[8:] for r in press.encode_records(list(sig), hdrs)]
    bad = bytearray(recs[3])
    bad[-1] ^= 0x5A                                                        # the Adler-32 of the zlib stream
    recs[3] = bytes(bad)
    caps = [4000, 96, 4008, 4000, 4003]
    dec = press.decode_to_device(recs, sig_caps=caps)
    f = dec.t_fields.cpu().numpy().view(gpu.lib.REC_FIELDS)[:5].copy()
    assert f["status"].tolist()[:3] == [0, 6, 0] and f["status"][3] != 0 and f["status"][4] == 0
    assert int(f["n_samples"][1]) == 4000                                  # larger than the slot: what a kernel must not trust
    h = dec.t_sig.cpu().numpy()
    slots = [h[int(o):int(o) + c] for o, c in zip(dec.sig_off, caps)]
    b = Batch(slots, caps, f)
    stats, dev = _run_stats(gpu, b)
    for i in (0, 2, 4):
        assert int(stats["status"][i]) == 0
        assert_stats_equal(stats[i], stats_ref(sig[i]), i)
    for i in (1, 3):
        assert int(stats["status"][i]) == int(f["status"][i]) != 0
        assert_stats_equal(stats[i], stats_ref([]), i)
    # a window on a failed read: zeros and a status, nothing loaded
    out, wst = _run_windows(gpu, b, dev, np.array([1, 3, 0], np.uint32), np.array([0, 0, 0], np.uint32), 64, "medmad", np.float32)
    assert wst.tolist() == [1, 1, 0] and (out[:2] == 0).all() and (out[2] != 0).any()
    # the device path through read_signals and the chunk call agree on the same records
    st2 = signals.signal_stats(recs, quantiles=QUANTILES, raise_on_error=False)
    for i in (0, 2, 4):
        assert_stats_equal(st2[i], stats_ref(sig[i]), i)
    assert int(st2["status"][3]) == int(f["status"][3]) and int(st2["n"][3]) == 0
    assert int(st2["status"][1]) == 0                                      # (the chunk call sizes its own slots)


def _run_windows(env, b, dev, wr, ws, W, mode, np_dtype, a=0.51, bq=0.53):
    """k_sig_windows with guard elements in front of and behind `out` -> (rows, win_status)"""
    torch, L, S = env.torch, env.L, env.signals
    d_sig, d_off, d_cap, d_f, d_st, pad = dev
    nw = len(wr)
    t_dtype = torch.float16 if np_dtype == np.float16 else torch.float32
    G = 64
    out = torch.full((G + nw * W + G,), 12352.0, dtype=t_dtype, device="cuda")
    d_wr = torch.from_numpy(np.ascontiguousarray(wr).view(np.int32).copy()).to("cuda")
    d_ws = torch.from_numpy(np.ascontiguousarray(ws).view(np.int32).copy()).to("cuda")
    d_wst = torch.full((nw + 2,), -7, dtype=torch.int32, device="cuda")
    env.lib.check(L.s5gpu_signal_windows_dev(b.n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), d_st.data_ptr() + pad,
                                             nw, d_wr.data_ptr(), d_ws.data_ptr(), W, S.NORMS[mode], a, bq,
                                             env.lib.SIG_F16 if np_dtype == np.float16 else env.lib.SIG_F32,
                                             out.data_ptr() + G * out.element_size(), d_wst.data_ptr() + 4, None), "s5gpu_signal_windows_dev")
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[:G] == 12352.0).all() and (h[G + nw * W:] == 12352.0).all(), "guard elements around out"
    wst = d_wst.cpu().numpy()
    assert wst[0] == -7 and wst[-1] == -7
    return h[G:G + nw * W].reshape(nw, W), wst[1:-1]


def _half_ord(h):
    """float16 -> integers in the order of the values (for a distance in ulps)"""
    u = np.asarray(h, dtype=np.float16).view(np.uint16).astype(np.int32)
    return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)


def _expected_rows(env, b, stats, wr, ws, W, mode):
    """float64 rows of the restatement, the row's count of real samples, and the expected win_status"""
    rows = np.zeros((len(wr), W), dtype=np.float64)
    cnt, bad = np.zeros(len(wr), dtype=np.int64), np.zeros(len(wr), dtype=np.int32)
    cache = {}
    for w, (r, s) in enumerate(zip(wr.tolist(), ws.tolist())):
        if r >= b.n or b.fields["status"][r] != 0 or s > min(len(b.reads[r]), int(b.cap[r])):
            bad[w] = 1
            continue
        if r not in cache:
            cache[r] = norm_ref(b.reads[r], mode, b.fields[r], stats[r])
        seg = cache[r][s:s + W]
        rows[w, :len(seg)] = seg
        cnt[w] = len(seg)
    return rows, cnt, bad


def _check_windows(env, b, stats, dev, wr, ws, W, mode, np_dtype):
    got, wst = _run_windows(env, b, dev, wr, ws, W, mode, np_dtype)
    rows, cnt, bad = _expected_rows(env, b, stats, wr, ws, W, mode)
    assert np.array_equal(wst, bad)
    pad = np.arange(W)[None, :] >= cnt[:, None]
    assert (got[pad] == 0).all()                                           # padding and refused rows: exactly 0
    want32 = rows.astype(np.float32)
    if np_dtype == np.float16:
        d = np.abs(_half_ord(got) - _half_ord(want32.astype(np.float16)))
        assert d.max() <= 1, (mode, int(d.max()))                          # within one float16 ulp of float16(float32 result)
    elif mode in ("raw", "pa"):
        assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), mode      # bit-equal
    else:
        np.testing.assert_allclose(got.astype(np.float64), rows, rtol=1e-6, atol=0)
    return got


def _mixed_plan(env, W, ov):
    b = env.batch
    wr, ws = env.signals.chunk_plan([len(x) for x in b.reads], W, ov)
    long_read = max(range(b.n), key=lambda i: len(b.reads[i]))
    extra_r = np.array([b.n, 0xFFFFFFFF, long_read, long_read, 3], dtype=np.uint32)
    extra_s = np.array([0, 0, len(b.reads[long_read]) + 1, len(b.reads[long_read]), 0xFFFFFFFF], dtype=np.uint32)
    return np.concatenate([wr, extra_r]), np.concatenate([ws, extra_s])    # ... and descriptors out of range (one of them just in range)


@pytest.mark.gpu
@pytest.mark.parametrize("np_dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("mode", ["raw", "pa", "medmad", "quant"])
def test_windows_in_every_mode(gpu, gpu_stats, mode, np_dtype):
    stats, dev = gpu_stats
    wr, ws = _mixed_plan(gpu, 64, 8)
    got = _check_windows(gpu, gpu.batch, stats, dev, wr, ws, 64, mode, np_dtype)
    if mode == "medmad":                                                   # a constant read: mad4 = 0, scale 1, every value 0
        const = [i for i, x in enumerate(gpu.batch.reads) if len(x) > 1 and (x == x[0]).all()]
        assert const and all(int(stats["mad4"][i]) == 0 for i in const)
        assert (got[np.isin(wr, const)] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("np_dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_windows_of_an_odd_width_and_the_padded_batch(gpu, gpu_stats, np_dtype):
    """W = 13: rows start at any alignment and the tensor's last chunk is partial; then the padded [n, T] batch (r_w = w, s_w = 0)"""
    stats, dev = gpu_stats
    b = gpu.batch
    wr, ws = gpu.signals.chunk_plan([len(x) if len(x) < 300 else 0 for x in b.reads], 13, 3)
    wr, ws = np.concatenate([wr, np.array([b.n + 5], np.uint32)]), np.concatenate([ws, np.array([0], np.uint32)])
    if (len(wr) * 13) % 8 == 0:
        wr, ws = wr[1:], ws[1:]
    assert (len(wr) * 13) % 8 != 0
    for mode in ("raw", "pa", "medmad", "quant"):
        _check_windows(gpu, b, stats, dev, wr, ws, 13, mode, np_dtype)
    n = 40
    small = Batch(b.reads[:n], b.cap[:n], b.fields[:n].copy())             # T = 4100: longer reads are cut there, shorter ones padded
    st, dv = _run_stats(gpu, small)
    _check_windows(gpu, small, st, dv, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), 4100, "medmad", np_dtype)


E2E_FILES = ["exp_1_lossless_zlib_svb_v0.2.0.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5", "exp_1_lossless_zlib_ex_zd.blow5", "exp_1_lossless.blow5",
             "example_multi_rg_v0.2.0.blow5"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E_FILES)
def test_read_signals_on_golden_files(gpu, name):
    """every read, reassembled from its windows, is numpy's normalisation of the signal press.decode_records returns for it"""
    torch, press, signals = gpu.torch, gpu.press, gpu.signals
    f = Blow5(golden(name))
    want = press.decode_records(f.records, f.rec_method, f.sig_method)
    W, ov = 512, 64
    for norm, dtype in (("medmad", torch.float32), ("pa", torch.float32), ("raw", torch.float16), ("quant", torch.float32)):
        out, wr, ws, stats, fields = signals.read_signals(f.records, f.rec_method, f.sig_method, norm=norm, window=W, overlap=ov, dtype=dtype)
        assert out.is_cuda and tuple(out.shape) == (len(wr), W)
        h = out.cpu().numpy()
        for i, g in enumerate(want):
            x = g["signal"]
            assert int(stats["status"][i]) == 0 and int(fields["n_samples"][i]) == len(x)
            assert_stats_equal(stats[i], stats_ref(x, (0.2, 0.9)), (name, i))
            ref = norm_ref(x, norm, g, stats_ref(x, (0.2, 0.9)))
            rebuilt = np.full(len(x), np.nan)
            for w in np.nonzero(wr == i)[0]:
                m = min(W, len(x) - int(ws[w]))
                rebuilt[int(ws[w]):int(ws[w]) + m] = h[w, :m]
                assert (h[w, m:] == 0).all()
            if norm == "pa":
                assert np.array_equal(rebuilt.astype(np.float32).view(np.uint32), ref.astype(np.float32).view(np.uint32))
            elif norm == "raw":
                assert np.array_equal(rebuilt, x.astype(np.float16).astype(np.float64))
            else:
                np.testing.assert_allclose(rebuilt, ref, rtol=1e-6, atol=0)
    # the padded batch: one row per read
    out, wr, ws, stats, fields = signals.read_signals(f.records, f.rec_method, f.sig_method, norm="raw")
    h = out.cpu().numpy()
    assert h.shape == (len(want), max(len(g["signal"]) for g in want))
    for i, g in enumerate(want):
        assert np.array_equal(h[i, :len(g["signal"])], g["signal"].astype(np.float32)) and (h[i, len(g["signal"]):] == 0).all()


@pytest.mark.gpu
def test_chunk_call_matches_the_device_path_and_reports_a_corrupt_record(gpu):
    signals, press = gpu.signals, gpu.press
    f = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    assert len(f.records) >= 2
    want = press.decode_records(f.records, f.rec_method, f.sig_method)
    st, fl = signals.signal_stats(f.records, f.rec_method, f.sig_method, quantiles=QUANTILES, with_fields=True)
    _, _, _, st_dev, _ = signals.read_signals(f.records, f.rec_method, f.sig_method, norm="raw", quantiles=QUANTILES)
    assert st.tobytes() == st_dev.tobytes()
    for i, g in enumerate(want):
        assert int(st["status"][i]) == 0 and int(fl["n_samples"][i]) == len(g["signal"])
        assert_stats_equal(st[i], stats_ref(g["signal"]), i)
    recs = list(f.records)
    bad = bytearray(recs[1])
    bad[-1] ^= 0x5A
    recs[1] = bytes(bad)
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        signals.signal_stats(recs, f.rec_method, f.sig_method)
    st, fl = signals.signal_stats(recs, f.rec_method, f.sig_method, quantiles=QUANTILES, raise_on_error=False, with_fields=True)
    assert int(st["status"][1]) == int(fl["status"][1]) != 0 and int(st["n"][1]) == 0
    assert_stats_equal(st[0], stats_ref(want[0]["signal"]), 0)
    # a pair of methods the no-payload decoder does not serve goes through the full decode
    g = Blow5(golden("exp_1_lossless.blow5"))
    st = signals.signal_stats(g.records, g.rec_method, g.sig_method, quantiles=QUANTILES)
    for i, d in enumerate(press.decode_records(g.records, g.rec_method, g.sig_method)):
        assert_stats_equal(st[i], stats_ref(d["signal"]), i)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(gpu, gpu_stats):
    L, S = gpu.L, gpu.signals
    _, (d_sig, d_off, d_cap, d_f, d_st, pad) = gpu_stats
    n = gpu.batch.n
    before = d_st.cpu().numpy().copy()
    q5 = (C.c_double * 5)(0.1, 0.2, 0.3, 0.4, 0.5)
    assert L.s5gpu_signal_stats_dev(n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), 5, q5, d_st.data_ptr() + pad, None) == -1
    assert b"quantiles" in L.s5gpu_last_error()
    for bad_q in (1.5, -0.1, float("nan")):
        q = (C.c_double * 1)(bad_q)
        assert L.s5gpu_signal_stats_dev(n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), 1, q, d_st.data_ptr() + pad, None) == -1
        assert L.s5gpu_signal_stats_stream(1, None, 0, None, None, 1, 1, 1, q, None, None) == -1
    out = gpu.torch.full((4 * 64,), 7.0, dtype=gpu.torch.float32, device="cuda")
    wr = gpu.torch.zeros(4, dtype=gpu.torch.int32, device="cuda")
    wst = gpu.torch.full((4,), -7, dtype=gpu.torch.int32, device="cuda")

    def windows(W=64, mode=0, dtype=0):
        return L.s5gpu_signal_windows_dev(n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), d_st.data_ptr() + pad, 4,
                                          wr.data_ptr(), wr.data_ptr(), W, mode, 0.51, 0.53, dtype, out.data_ptr(), wst.data_ptr(), None)
    assert windows(W=0) == -1 and windows(mode=4) == -1 and windows(mode=-1) == -1 and windows(dtype=2) == -1
    gpu.torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all() and (wst.cpu().numpy() == -7).all()          # nothing was launched
    assert np.array_equal(d_st.cpu().numpy(), before)
    assert windows() == 0
    gpu.torch.cuda.synchronize()
    assert (wst.cpu().numpy() == 0).all()
