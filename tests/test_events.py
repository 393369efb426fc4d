"""events: scrappie-style event segmentation of decoded reads on the device (docs/codecs.md §4.15; slow5tools_amd/csrc/event_kernels.hip).

The oracle is a numpy / Python restatement of §4.15 kept in this file: the exact t-statistic on integers, the two-detector peak machine, the
events between the sorted peaks and the float64 row arithmetic.  The device is held to it exactly: start, length and the counts as integers,
mean and stdv bit for bit as float32.  The walk a lane runs (event_dev.h) is plain C++: it is also compiled for the CPU and held to the same
oracle, so a wrong slot counter or window sum shows without a device.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import Blow5, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DNA = (3, 6, 1.4, 9.0, 0.2)
RNA = (7, 14, 2.5, 9.0, 1.0)
W64 = (3, 64, 1.4, 9.0, 0.2)                                              # the widest long window: the largest ring
BOTH = (3, 6, 8.0, 4.0, 0.2)                                              # thresholds at which the LONG detector emits too (with DNA's it never gets to)
LENGTHS = [0, 1, 2, 5, 6, 11, 12, 13, 27, 28, 63, 64, 65, 255, 256, 257, 4000, 4097, 70001]
KINDS = ["levels_sd0", "levels_sd3", "levels_sd12", "constant", "extremes", "ramp", "multiples_of_8", "synth"]
GUARD = 0x2AAB
RAW, PA = 0, 1
EVENT = np.dtype([("start", "<u4"), ("length", "<u4"), ("mean", "<f4"), ("stdv", "<f4")])
E2E_FILES = ["exp_1_lossless.blow5", "exp_1_lossless_zlib_svb_v0.2.0.blow5", "exp_1_lossless_zstd_svb_v0.2.0.blow5", "exp_1_lossless_zlib_ex_zd.blow5"]


# ---------------------------------------------------------------------------------------------------------------- the restatement

def t_stat(x, w, with_floored=False):
    """t_w[i] of §4.15 for every i: sqrt(num / den) on integers, one division and one square root in float64; 0 where a window does not fit.
    with_floored: also the positions where the variance floor (den >= 1) was used"""
    x = np.asarray(x).astype(np.int64)
    n = len(x)
    t = np.zeros(n, dtype=np.float64)
    if n < 2 * w:
        return (t, np.zeros(n, dtype=bool)) if with_floored else t
    P = np.concatenate([[0], np.cumsum(x)])
    Q = np.concatenate([[0], np.cumsum(x * x)])
    i = np.arange(w, n - w + 1)
    s1, s2 = P[i] - P[i - w], P[i + w] - P[i]
    q1, q2 = Q[i] - Q[i - w], Q[i + w] - Q[i]
    num = (s2 - s1) ** 2 * w
    den = np.maximum(w * (q1 + q2) - (s1 * s1 + s2 * s2), 1)
    assert num.max(initial=0) < 2 ** 53 and den.max(initial=0) < 2 ** 53 and den.min(initial=1) >= 1
    t[i] = np.sqrt(num.astype(np.float64) / den.astype(np.float64))
    if with_floored:
        floored = np.zeros(n, dtype=bool)
        floored[i] = w * (q1 + q2) - (s1 * s1 + s2 * s2) < 1
        return t, floored
    return t


def peaks(x, params, who=None):
    """the positions the two detectors emit, in the order of emission; asserts that the order is strictly increasing on every input.
    who: a list that gets the detector (0 short, 1 long) of every emission"""
    w1, w2, thr1, thr2, ph = params
    n = len(x)
    t = [t_stat(x, w1).tolist(), t_stat(x, w2).tolist()]
    w, thr = (w1, w2), (thr1, thr2)
    inf = float("inf")
    masked, pos, val, valid = [0, 0], [None, None], [inf, inf], [False, False]
    out = []
    for i in range(n):
        for k in (0, 1):
            if masked[k] >= i:
                continue
            c = t[k][i]
            if pos[k] is None:
                if c < val[k]:
                    val[k] = c
                elif c - val[k] > ph:
                    val[k] = c
                    pos[k] = i
            else:
                if c > val[k]:
                    val[k] = c
                    pos[k] = i
                if k == 0 and val[0] > thr1:
                    masked[1] = pos[0] + w1
                    pos[1], val[1], valid[1] = None, inf, False
                if val[k] - c > ph and val[k] > thr[k]:
                    valid[k] = True
                if valid[k] and i - pos[k] > w[k] // 2:
                    assert not out or pos[k] > out[-1], "a peak was emitted at or in front of the one before it"
                    out.append(pos[k])
                    if who is not None:
                        who.append(k)
                    pos[k], val[k], valid[k] = None, c, False
    return out


def events_ref(x, params, mode=RAW, f=None):
    """the EVENT rows of one read: events between the sorted set of peaks, float64 arithmetic with every operation rounded on its own"""
    x = np.asarray(x).astype(np.int64)
    n = len(x)
    if n == 0:
        return np.zeros(0, dtype=EVENT)
    b = np.array([0] + sorted(set(peaks(x, params))) + [n], dtype=np.int64)
    P = np.concatenate([[0], np.cumsum(x)])
    Q = np.concatenate([[0], np.cumsum(x * x)])
    L = np.diff(b)
    S, QQ = P[b[1:]] - P[b[:-1]], Q[b[1:]] - Q[b[:-1]]
    Ld = L.astype(np.float64)
    mean = S.astype(np.float64) / Ld
    m2 = mean * mean
    var = QQ.astype(np.float64) / Ld - m2
    sd = np.sqrt(np.maximum(var, 0.0))
    out = np.zeros(len(L), dtype=EVENT)
    out["start"], out["length"] = b[:-1], L
    if mode == PA:
        s = np.float64(f["range"]) / np.float64(f["digitisation"])
        out["mean"], out["stdv"] = ((mean + np.float64(f["offset"])) * s).astype(np.float32), (sd * np.abs(s)).astype(np.float32)
    else:
        out["mean"], out["stdv"] = mean.astype(np.float32), sd.astype(np.float32)
    return out


def levels(n, sd, rng, with_bounds=False):
    """random levels of dwell 4 .. 20 with Gaussian noise of standard deviation sd"""
    lv, bounds = [], []
    while len(lv) < n:
        if lv:
            bounds.append(len(lv))
        lv += [int(rng.integers(300, 700))] * int(rng.integers(4, 21))
    a = np.array(lv[:n], dtype=np.float64)
    if sd:
        a = a + rng.normal(0.0, sd, n)
    x = np.round(a).astype(np.int16)
    return (x, [p for p in bounds if p < n]) if with_bounds else x


def _contents(n, kind, rng):
    if kind.startswith("levels_sd"):
        return levels(n, int(kind[9:]), rng)
    if kind == "constant":
        return np.full(n, 517, dtype=np.int16)
    if kind == "extremes":
        return np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    if kind == "ramp":
        return (np.arange(n, dtype=np.int64) % 65536 - 32768).astype(np.int16)
    if kind == "multiples_of_8":                                           # a degraded file
        return (levels(n, 5, rng).astype(np.int32) // 8 * 8).astype(np.int16)
    return ob.synth_reads(0x5105, n % 97, 1, n)[0] if n else np.zeros(0, np.int16)


# ---------------------------------------------------------------------------------------------------------------- not gpu

def test_library_exports_the_event_calls():
    from slow5tools_amd import _lib

    names = ["s5gpu_signal_events_dev", "s5gpu_signal_events_batch"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert not [s for s in names if s not in exported]
    assert not [s for s in names if s not in _lib.EXPORTS]
    L = _lib.lib()
    assert len(L.s5gpu_signal_events_dev.argtypes) == 13 and len(L.s5gpu_signal_events_batch.argtypes) == 11


def test_event_layouts_match_header(tmp_path):
    from slow5tools_amd import _lib, events

    ev, pr = ["start", "length", "mean", "stdv"], ["w1", "w2", "thr1", "thr2", "peak_height"]
    src = tmp_path / "ly.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slow5gpu.h"\nint main(void){printf("%zu", sizeof(s5gpu_event_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_event_t, %s));\n' % m for m in ev)
                   + 'printf(" %zu", sizeof(s5gpu_event_params_t));\n'
                   + "".join('printf(" %%zu", offsetof(s5gpu_event_params_t, %s));\n' % m for m in pr)
                   + 'printf(" %d\\n", S5GPU_STATUS_EVENTS_OVERFLOW);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "ly")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "ly")], text=True).split()]
    D, Pm = events.EVENT, _lib.EventParams
    assert got == [D.itemsize] + [D.fields[m][1] for m in ev] + [C.sizeof(Pm)] + [getattr(Pm, m).offset for m in pr] + [_lib.STATUS_EVENTS_OVERFLOW]
    assert D.itemsize == 16 and D == EVENT and events.DNA == DNA and events.RNA == RNA


def test_s5events_exists_after_build():
    from slow5tools_amd import build, events

    build.build()
    assert os.access(events.S5EVENTS, os.X_OK)


def test_restatement_is_pinned_on_the_first_golden_read():
    f = Blow5(golden("exp_1_lossless.blow5"))
    assert (f.rec_method, f.sig_method) == (0, 0)
    x = ob.rec_parse(f.records[0], ob.SIG_NONE)["signal"]
    assert len(x) == 59676
    assert len(events_ref(x, DNA)) == 11908
    p = peaks(x, RNA)
    assert len(p) == 5200 and len(events_ref(x, RNA)) == 5201


def test_restatement_on_small_and_degenerate_reads():
    assert peaks([0] * 50 + [1] * 50, DNA) == [50]
    assert len(events_ref(np.full(300, 5), DNA)) == 1
    assert len(events_ref(np.where(np.arange(400) % 2 == 0, 32767, -32768), DNA)) == 1
    for n in range(1, 6):
        e = events_ref(np.arange(n) * 100, DNA)
        assert len(e) == 1 and (int(e["start"][0]), int(e["length"][0])) == (0, n)
    assert len(events_ref([], DNA)) == 0
    e = events_ref([0] * 50 + [1] * 50, DNA)
    assert e["start"].tolist() == [0, 50] and e["length"].tolist() == [50, 50] and e["mean"].tolist() == [0.0, 1.0] and e["stdv"].tolist() == [0.0, 0.0]


def test_restatement_is_invariant_under_an_affine_map():
    """x -> 3 x + 100 multiplies num and den by 9, both still exact integers, so the quotient rounds to the same double.  The variance floor is
    one RAW unit and does not scale: where two windows are each constant the statistic grows with the map, so the equality is asserted where
    the floor is not used, and the peaks are compared on reads that never use it"""
    rng = np.random.default_rng(11)
    whole = 0
    for trial in range(6):
        x = levels(1500, 12, rng).astype(np.int64)
        y = 3 * x + 100                                                     # exact in int64 and inside int16
        assert y.max() < 32768
        for pr in (DNA, RNA):
            clean = True
            for w in pr[:2]:
                (tx, fx), (ty, fy) = t_stat(x, w, True), t_stat(y, w, True)
                assert np.array_equal(fx, fy) and np.array_equal(tx[~fx], ty[~fx]) and fx.mean() < 0.01
                clean &= not fx.any()
            if clean:
                assert peaks(x, pr) == peaks(y, pr) and len(peaks(x, pr)) > 50
                whole += 1
    assert whole >= 6


def test_restatement_emits_strictly_increasing_peaks_and_finds_the_boundaries():
    rng = np.random.default_rng(3)
    for trial in range(60):                                                # (peaks() asserts the order on every input it is given)
        n = int(rng.integers(0, 500))
        x = rng.integers(-40, 40, n) + np.cumsum(rng.integers(-500, 500, n) * (rng.random(n) < 0.1))
        for pr in (DNA, RNA, (1, 2, 0.5, 1.0, 0.1), (3, 64, 1.0, 2.0, 0.2)):
            p = peaks(np.clip(x, -32768, 32767), pr)
            assert p == sorted(set(p))
    # against a vacuous pass: the noisy levels give at least one event per 20 samples, and without noise the true boundaries are found
    for sd in (3, 12):
        assert len(peaks(levels(4000, sd, rng), DNA)) >= 200
    for sd in (3, 12):                                                     # both detectors at work
        who = []
        peaks(levels(4000, sd, rng), BOTH, who)
        assert who.count(0) >= 100 and who.count(1) >= 10
    x, bounds = levels(4000, 0, rng, with_bounds=True)
    true = [b for b in bounds if x[b] != x[b - 1]]
    found = set(peaks(x, DNA))
    assert len(true) >= 250 and len([b for b in true if b in found]) >= 0.95 * len(true)


WALK_HOST = r'''
// One lane's walk (event_dev.h) on the CPU: in.bin holds cases, out.bin gets a count and the rows of each.  The ring column has a pitch of 3
// and guard words between and around its slots; the rows have a guard row on either side.
#define S5_EVENT_WALK_HOST
#include "event_dev.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (argc != 3 || !f || !o) return 1;
    for (;;) {
        uint32_t w[2], mis, n, extra; double th[3], os[2]; int32_t mode;
        if (fread(w, 4, 2, f) != 2) break;
        if (fread(th, 8, 3, f) != 3 || fread(&mode, 4, 1, f) != 1 || fread(&mis, 4, 1, f) != 1 || fread(os, 8, 2, f) != 2 || fread(&n, 4, 1, f) != 1 ||
            fread(&extra, 4, 1, f) != 1) return 1;
        int16_t *buf = (int16_t *)aligned_alloc(16, (2 * (size_t)(n + 16) + 31) / 16 * 16);
        int16_t *p = buf + mis;
        if (fread(p, 2, n, f) != n) return 1;
        evk::EvArgs A = {w[0], w[1], th[0], th[1], th[2], mode, 0, 0, 0, 0, 0};
        const uint32_t ring = evk::ring_slots(w[1]), pitch = 3;
        std::vector<int16_t> col((size_t)ring * pitch + 8, 0x7777);
        evk::RowOut O0 = {nullptr, 0, false, 0, 1};
        const uint32_t c0 = evk::walk<false>(p, n, n + extra, mis % 8 == 0, col.data() + 1, pitch, ring, A, O0);
        std::vector<evk::U4> rows(c0 + 2);
        memset(rows.data(), 0xEE, 16 * rows.size());
        evk::RowOut O = {rows.data() + 1, c0, mode == 1, os[0], os[1]};
        const uint32_t c1 = evk::walk<true>(p, n, n + extra, mis % 8 == 0, col.data() + 1, pitch, ring, A, O);
        for (size_t k = 0; k < col.size(); k++)
            if ((k < 1 || (k - 1) % pitch != 0 || (k - 1) / pitch >= ring) && col[k] != 0x7777) { fprintf(stderr, "a word outside the ring was written\n"); return 2; }
        if (c1 != c0 || rows[0].x != 0xEEEEEEEEu || rows[c0 + 1].x != 0xEEEEEEEEu) { fprintf(stderr, "counts differ or a guard row was written\n"); return 3; }
        fwrite(&c0, 4, 1, o); fwrite(rows.data() + 1, 16, c0, o);
        free(buf);
    }
    return fclose(o) == 0 ? 0 : 1;
}
'''


def test_the_lane_walk_compiled_for_the_cpu_matches_the_restatement(tmp_path):
    """the code a lane of k_sig_events runs, with a misaligned read (the 2-byte loads), a wave that walks past the read's end (`extra`), both
    modes and the four parameter sets"""
    rng = np.random.default_rng(5)
    f = dict(offset=13.0, range=1467.61, digitisation=8192.0)
    cases = []
    for n in [0, 1, 2, 5, 6, 11, 12, 13, 27, 28, 63, 64, 65, 255, 256, 257, 1000]:
        for j, kind in enumerate(KINDS[:7]):
            cases.append((_contents(n, kind, rng), (DNA, RNA, W64, BOTH)[(n + j) % 4], (n + j) % 2, int(rng.integers(0, 9)), int(rng.integers(0, 100))))
    with open(tmp_path / "in.bin", "wb") as fh:
        for x, pr, mode, mis, extra in cases:
            fh.write(struct.pack("<IIdddiIddII", pr[0], pr[1], pr[2], pr[3], pr[4], mode, mis, f["offset"], f["range"] / f["digitisation"], len(x), extra))
            fh.write(x.tobytes())
    (tmp_path / "walk_host.cpp").write_text(WALK_HOST)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "slow5tools_amd", "csrc"),
                           str(tmp_path / "walk_host.cpp"), "-o", str(tmp_path / "walk_host")])
    subprocess.check_call([str(tmp_path / "walk_host"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw, at, n_events = (tmp_path / "out.bin").read_bytes(), 0, 0
    for x, pr, mode, mis, extra in cases:
        c = struct.unpack_from("<I", raw, at)[0]
        got = np.frombuffer(raw, EVENT, c, at + 4)
        at += 4 + 16 * c
        want = events_ref(x, pr, mode, f)
        assert got.tobytes() == want.tobytes(), (len(x), pr, mode, mis, extra)
        n_events += c
    assert at == len(raw) and n_events > 500


# ---------------------------------------------------------------------------------------------------------------- gpu

class Batch:
    """reads laid out as the decoder would leave them, with guard words between the slots; every fifth slot starts off the 16-byte grid"""

    def __init__(self, reads, caps, fields):
        self.reads, self.n = reads, len(reads)
        self.cap = np.asarray(caps, dtype=np.uint32)
        self.fields = fields
        pos, offs = 16, []
        for i, c in enumerate(self.cap):
            offs.append(pos + (3 if i % 5 == 4 else 0))
            pos += (int(c) + 7) // 8 * 8 + 8 * (1 + i % 3)
        self.off = np.asarray(offs, dtype=np.uint64)
        self.base = np.full(pos + 16, GUARD, dtype=np.int16)
        for o, c, x in zip(offs, self.cap, reads):
            self.base[o:o + int(c)] = -1234                                # slot space behind the samples
            m = min(len(x), int(c))
            self.base[o:o + m] = x[:m]


def _golden_fields():
    g = ob.rec_parse(Blow5(golden("exp_1_lossless.blow5")).records[0], ob.SIG_NONE)
    assert g["digitisation"] == 8192.0 and abs(g["range"] - 1467.61) < 1e-2
    return g


@pytest.fixture(scope="module")
def gpu():
    """the library initialised and the mixed batch; reference rows are made once per (parameters, mode) and shared"""
    import torch
    from slow5tools_amd import _lib, events, press

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
    env = type("Env", (), {})()
    env.torch, env.lib, env.L, env.press, env.events, env.batch = torch, _lib, _lib.lib(), press, events, Batch(reads, caps, fields)
    env.kind = [KINDS[(i + j) % len(KINDS)] for j in range(len(KINDS)) for i, n in enumerate(LENGTHS)]
    env.cache = {}

    def ref(params, mode):
        if (params, mode) not in env.cache:
            env.cache[(params, mode)] = [events_ref(x, params, mode, fields[i]) for i, x in enumerate(reads)]
        return env.cache[(params, mode)]
    env.ref = ref
    return env


def _run_events(env, b, params, mode, caps=None, count_only=False):
    """the count pass, then the fill pass into slots of caps[i] rows (default: the counts) with guard rows between and around them ->
    dict(count, count_status, n_events, status, rows: list of EVENT arrays of min(n_events, cap) rows).  Guards are checked here."""
    torch, L = env.torch, env.L
    n = b.n
    d_sig = torch.from_numpy(b.base.copy()).to("cuda")
    d_off = torch.from_numpy(b.off.view(np.int64).copy()).to("cuda")
    d_cap = torch.from_numpy(b.cap.view(np.int32).copy()).to("cuda")
    d_f = torch.from_numpy(b.fields.view(np.uint8).copy()).to("cuda")
    p = env.lib.EventParams(*params)

    def call(ev_off, ev_cap, rows):
        d_cnt = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
        d_st = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
        env.lib.check(L.s5gpu_signal_events_dev(n, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), C.byref(p), mode,
                                                ev_off, ev_cap, rows, d_cnt.data_ptr() + 4, d_st.data_ptr() + 4, None), "s5gpu_signal_events_dev")
        torch.cuda.synchronize()
        c, s = d_cnt.cpu().numpy(), d_st.cpu().numpy()
        assert c[0] == c[-1] == s[0] == s[-1] == -7, "guard words around n_events / ev_status"
        return c[1:-1].view(np.uint32).copy(), s[1:-1].copy()
    out = {}
    out["count"], out["count_status"] = call(None, None, None)
    if count_only:
        return out
    caps = out["count"] if caps is None else np.asarray(caps, dtype=np.uint32)
    pos, offs = 2, []
    for i, c in enumerate(caps):
        offs.append(pos)
        pos += int(c) + 1 + i % 3
    ev_off = np.asarray(offs, dtype=np.uint64)
    host = np.full((pos + 2) * 16, 0xA5, dtype=np.uint8)
    d_rows = torch.from_numpy(host.copy()).to("cuda")
    d_eo = torch.from_numpy(ev_off.view(np.int64).copy()).to("cuda")
    d_ec = torch.from_numpy(caps.view(np.int32).copy()).to("cuda")
    out["n_events"], out["status"] = call(d_eo.data_ptr(), d_ec.data_ptr(), d_rows.data_ptr())
    got = d_rows.cpu().numpy()
    written = np.zeros(pos + 2, dtype=bool)
    out["rows"] = []
    for i in range(n):
        m = min(int(out["n_events"][i]), int(caps[i]))
        written[offs[i]:offs[i] + m] = True
        out["rows"].append(got.view(EVENT)[offs[i]:offs[i] + m].copy())
    assert (got.reshape(-1, 16)[~written] == 0xA5).all(), "a row outside [ev_off, ev_off + min(n_events, ev_cap)) was written"
    assert np.array_equal(d_sig.cpu().numpy(), b.base), "k_sig_events wrote to the signals"
    return out


@pytest.fixture(scope="module")
def gpu_runs(gpu):
    """every device run over the mixed batch, made once: DNA and RNA in both modes, the widest window and the both-detector thresholds raw"""
    return {(pr, mode): _run_events(gpu, gpu.batch, pr, mode) for pr, mode in ((DNA, RAW), (DNA, PA), (RNA, RAW), (RNA, PA), (W64, RAW), (BOTH, RAW))}


@pytest.mark.gpu
@pytest.mark.parametrize("params", [DNA, RNA, W64, BOTH], ids=["dna", "rna", "w2_64", "both_detectors"])
def test_starts_lengths_and_counts_are_exact_over_a_mixed_batch(gpu, gpu_runs, params):
    r, want = gpu_runs[(params, RAW)], gpu.ref(params, RAW)
    for i, w in enumerate(want):
        what = (i, gpu.kind[i], len(gpu.batch.reads[i]))
        assert int(r["count"][i]) == int(r["n_events"][i]) == len(w), what       # rows = NULL counts what the fill pass fills
        assert int(r["count_status"][i]) == int(r["status"][i]) == 0, what
        assert np.array_equal(r["rows"][i]["start"], w["start"]) and np.array_equal(r["rows"][i]["length"], w["length"]), what
        if len(w):
            assert int(w["start"][0]) == 0 and int(w["start"][-1] + w["length"][-1]) == len(gpu.batch.reads[i])
    # against a vacuous pass: the noisy levels are cut at least once per 20 samples
    for i, w in enumerate(want):
        n = len(gpu.batch.reads[i])
        if gpu.kind[i] in ("levels_sd3", "levels_sd12") and n >= 255 and params != BOTH:
            assert len(w) >= n / 20, (i, n, len(w))


@pytest.mark.gpu
@pytest.mark.parametrize("params,mode", [(DNA, RAW), (DNA, PA), (RNA, RAW), (RNA, PA), (BOTH, RAW)],
                         ids=["dna-raw", "dna-pa", "rna-raw", "rna-pa", "both_detectors-raw"])
def test_mean_and_stdv_are_the_float64_restatement_bit_for_bit(gpu, gpu_runs, params, mode):
    r, want = gpu_runs[(params, mode)], gpu.ref(params, mode)
    n_rows = 0
    for i, w in enumerate(want):
        g = r["rows"][i]
        assert len(g) == len(w)
        for col in ("mean", "stdv"):
            bad = np.nonzero(g[col].view(np.uint32) != w[col].view(np.uint32))[0]
            assert len(bad) == 0, (i, gpu.kind[i], col, int(bad[0]), g[col][bad[0]], w[col][bad[0]])
        n_rows += len(w)
    assert n_rows > 10000


@pytest.mark.gpu
def test_failed_records_have_no_events_and_carry_their_status(gpu):
    """a real decode: one record into a signal slot that is too small (status 6, n_samples = the count it needed) and one corrupt record;
    the detector then runs over the decoder's slots rebuilt between guard words"""
    press = gpu.press
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
    b = Batch([h[int(o):int(o) + c] for o, c in zip(dec.sig_off, caps)], caps, f)
    r = _run_events(gpu, b, DNA, PA, caps=[1000] * 5)                      # (guards around every event slot and signal slot: checked in there)
    for i in (0, 2, 4):
        want = events_ref(sig[i], DNA, PA, f[i])
        assert int(r["status"][i]) == 0 and int(r["n_events"][i]) == len(want) > 100
        assert r["rows"][i].tobytes() == want.tobytes()
    for i in (1, 3):
        assert int(r["n_events"][i]) == int(r["count"][i]) == 0 and int(r["status"][i]) == int(r["count_status"][i]) == int(f["status"][i]) != 0
    # the device path of the Python layer on the same decode: the failed records have no rows
    rows, first = gpu.events.events_dev(dec, DNA, "pa")
    assert rows.is_cuda and rows.dtype == gpu.torch.int32 and tuple(rows.shape) == (int(first[-1]), 4)
    fi, hr = first.cpu().numpy(), rows.cpu().numpy()
    assert fi[2] == fi[1] and fi[4] == fi[3]
    for i in (0, 2, 4):
        assert hr[fi[i]:fi[i + 1]].tobytes() == events_ref(sig[i], DNA, PA, f[i]).tobytes()
    assert np.array_equal(rows[:, 2:].contiguous().view(gpu.torch.float32).cpu().numpy()[:, 0], hr.view(np.float32)[:, 2])


@pytest.mark.gpu
def test_overflow_keeps_the_true_count_and_fills_the_slot(gpu, gpu_runs):
    b, full = gpu.batch, gpu_runs[(DNA, RAW)]
    caps = full["count"] // 2
    r = _run_events(gpu, b, DNA, RAW, caps=caps)
    assert np.array_equal(r["n_events"], full["count"])
    for i in range(b.n):
        over = int(full["count"][i]) > int(caps[i])
        assert int(r["status"][i]) == (gpu.lib.STATUS_EVENTS_OVERFLOW if over else 0)
        assert r["rows"][i].tobytes() == full["rows"][i][:int(caps[i])].tobytes()
    assert sum(int(c) > 0 for c in full["count"]) - sum(int(s) != 0 for s in r["status"]) == 0    # every read with an event overflows: 1 // 2 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E_FILES)
def test_read_events_on_golden_files(gpu, name):
    f = Blow5(golden(name))
    want = gpu.press.decode_records(f.records, f.rec_method, f.sig_method)
    for params, mode in ((DNA, "raw"), (RNA, "pa")):
        rows, first, status = gpu.events.read_events(f.records, f.rec_method, f.sig_method, params=params, mode=mode)
        assert rows.dtype == EVENT and len(first) == len(want) + 1 and int(first[-1]) == len(rows) and not status.any()
        for i, g in enumerate(want):
            ref = events_ref(g["signal"], params, PA if mode == "pa" else RAW, g)
            assert rows[int(first[i]):int(first[i + 1])].tobytes() == ref.tobytes(), (name, i, params, mode)


@pytest.mark.gpu
def test_events_batch_nomem_protocol_then_success_and_a_corrupt_record(gpu):
    L, lib = gpu.L, gpu.lib
    f = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    recs = list(f.records)
    n = len(recs)
    assert n >= 2
    want = [events_ref(g["signal"], DNA) for g in gpu.press.decode_records(recs, f.rec_method, f.sig_method)]
    total = sum(len(w) for w in want)
    vp = C.c_void_p

    def batch(recs, room):
        rbuf = [C.create_string_buffer(r, max(len(r), 1)) for r in recs]
        rec_p = (vp * n)(*[C.addressof(b) for b in rbuf])
        rl = (C.c_size_t * n)(*[len(r) for r in recs])
        rows = np.full(room + 1, 0xA5, dtype=np.uint8).repeat(16).view(EVENT)
        first = np.full(n + 1, 77, dtype=np.uint64)
        st = np.full(n, -7, dtype=np.int32)
        p = lib.EventParams(*DNA)
        rc = L.s5gpu_signal_events_batch(n, rec_p, rl, f.rec_method, f.sig_method, C.byref(p), RAW, rows.ctypes.data_as(vp), room,
                                         first.ctypes.data_as(vp), st.ctypes.data_as(vp))
        return rc, rows, first, st
    rc, rows, first, st = batch(recs, total - 1)
    assert rc == -3 and int(first[0]) == total and (rows.view(np.uint8) == 0xA5).all()
    rc, rows, first, st = batch(recs, total)
    assert rc == 0 and int(first[0]) == 0 and int(first[n]) == total and not st.any() and (rows[total:].view(np.uint8) == 0xA5).all()
    for i, w in enumerate(want):
        assert rows[int(first[i]):int(first[i + 1])].tobytes() == w.tobytes()
    bad = bytearray(recs[1])
    bad[-1] ^= 0x5A
    recs[1] = bytes(bad)
    rc, rows, first, st = batch(recs, total)
    assert rc == -5 and st[1] != 0 and not st[0] and not st[2:].any() and first[2] == first[1]
    for i, w in enumerate(want):
        if i != 1:
            assert rows[int(first[i]):int(first[i + 1])].tobytes() == w.tobytes()
    with pytest.raises(lib.S5GpuError, match="rc=-5"):
        gpu.events.read_events(recs, f.rec_method, f.sig_method)
    ev, fi, st = gpu.events.read_events(recs, f.rec_method, f.sig_method, raise_on_error=False)
    assert st[1] != 0 and len(ev) == total - len(want[1])


def _lines(ids, rows):
    return b"".join(b"%s\t%d\t%d\t%d\t%s\t%s\n" % (rid, k, int(e["start"]), int(e["start"]) + int(e["length"]), b"%.6g" % float(e["mean"]), b"%.6g" % float(e["stdv"]))
                    for rid, ev in zip(ids, rows) for k, e in enumerate(ev))


@pytest.mark.gpu
def test_s5events_prints_the_restatements_lines(gpu, tmp_path):
    name = "exp_1_lossless_zlib_svb_v0.2.0.blow5"
    f = Blow5(golden(name))
    want = gpu.press.decode_records(f.records, f.rec_method, f.sig_method)
    ids = [g["read_id"] for g in want]
    for args, params, mode in (([], DNA, RAW), (["--pa"], DNA, PA), (["--rna", "-K", "1"], RNA, RAW)):
        p = subprocess.run([gpu.events.S5EVENTS] + args + [golden(name)], capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert p.stdout == _lines(ids, [events_ref(g["signal"], params, mode, g) for g in want]), args
    got_ids, got = gpu.events.file_events(golden(name))
    assert got_ids == ids and [len(e) for e in got] == [len(events_ref(g["signal"], DNA)) for g in want]
    # a corrupt record between good ones: its id on stderr, exit 1, the others printed
    m = Blow5(golden("example_multi_rg_v0.2.0.blow5"))
    raw = bytearray(m.raw)
    raw[m.offsets[1] + 8 + len(m.records[1]) - 1] ^= 0x5A
    (tmp_path / "bad.blow5").write_bytes(bytes(raw))
    want = gpu.press.decode_records(m.records, m.rec_method, m.sig_method)
    p = subprocess.run([gpu.events.S5EVENTS, str(tmp_path / "bad.blow5")], capture_output=True, timeout=120)
    assert p.returncode == 1 and want[1]["read_id"] in p.stderr
    keep = [g for i, g in enumerate(want) if i != 1]
    assert p.stdout == _lines([g["read_id"] for g in keep], [events_ref(g["signal"], DNA) for g in keep])
    assert subprocess.run([gpu.events.S5EVENTS], capture_output=True).returncode == 2


@pytest.mark.gpu
def test_refused_arguments_write_nothing(gpu):
    torch, L, lib, b = gpu.torch, gpu.L, gpu.lib, gpu.batch
    small = Batch(b.reads[:20], b.cap[:20], b.fields[:20].copy())
    d_sig = torch.from_numpy(small.base.copy()).to("cuda")
    d_off = torch.from_numpy(small.off.view(np.int64).copy()).to("cuda")
    d_cap = torch.from_numpy(small.cap.view(np.int32).copy()).to("cuda")
    d_f = torch.from_numpy(small.fields.view(np.uint8).copy()).to("cuda")
    d_cnt = torch.full((20,), -7, dtype=torch.int32, device="cuda")
    d_st = torch.full((20,), -7, dtype=torch.int32, device="cuda")

    def dev(params, mode=RAW, p_null=False):
        p = lib.EventParams(*params)
        return L.s5gpu_signal_events_dev(20, d_sig.data_ptr(), d_off.data_ptr(), d_cap.data_ptr(), d_f.data_ptr(), None if p_null else C.byref(p), mode,
                                         None, None, None, d_cnt.data_ptr(), d_st.data_ptr(), None)
    refused = [(3, 3, 1.4, 9.0, 0.2), (6, 3, 1.4, 9.0, 0.2), (3, 65, 1.4, 9.0, 0.2), (0, 6, 1.4, 9.0, 0.2), (3, 6, float("nan"), 9.0, 0.2),
               (3, 6, 1.4, float("inf"), 0.2), (3, 6, 1.4, 9.0, float("-inf"))]
    first = np.full(2, 77, dtype=np.uint64)
    rec = C.create_string_buffer(b"\0" * 16, 16)
    rec_p, rl = (C.c_void_p * 1)(C.addressof(rec)), (C.c_size_t * 1)(16)
    for pr in refused:
        assert dev(pr) == -1, pr
        p = lib.EventParams(*pr)
        assert L.s5gpu_signal_events_batch(1, rec_p, rl, 1, 1, C.byref(p), RAW, None, 0, first.ctypes.data_as(C.c_void_p), None) == -1, pr
    for mode in (2, 3, -1):
        assert dev(DNA, mode) == -1
        p = lib.EventParams(*DNA)
        assert L.s5gpu_signal_events_batch(1, rec_p, rl, 1, 1, C.byref(p), mode, None, 0, first.ctypes.data_as(C.c_void_p), None) == -1
    assert dev(DNA, p_null=True) == -1
    torch.cuda.synchronize()
    assert (d_cnt.cpu().numpy() == -7).all() and (d_st.cpu().numpy() == -7).all() and (first == 77).all()      # nothing was launched
    assert dev(DNA) == 0
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all() and (d_cnt.cpu().numpy() >= 0).all()
