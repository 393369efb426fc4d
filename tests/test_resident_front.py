"""The resident-decode front of the analysis calls (slow5tools_amd/csrc/host_ctx.h, resident_rules.h): one batch that holds a corrupt record
AND a record that outgrows the slot the decoder guessed for it, through every call that decodes and analyses.

The decoder redoes outgrown records itself, but stops at the first attempt that meets a corrupt one; the front then decodes the batch again
without the corrupt record.  So every call must return S5GPU_ERR_DATA, name itself in s5gpu_last_error(), give the corrupt record a status,
and give every other record — the outgrown one included — exactly what it gives for a batch of the five good records alone.
s5gpu_signal_stats_stream has no such second decode: what it does is pinned at the end.
"""
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from chain_common import levels_signal, record
from chain_common import gpu  # noqa: F401

ZS = (ob.REC_ZLIB, ob.SIG_SVB_ZD)
BAD, BIG = 2, 3                       # the truncated record and the one that outgrows its slot
GOOD = [0, 1, 3, 4, 5]
KW = dict(skip=1, qmax=64, qmin=10)
ERR_DATA = -5


class Batch:
    """six records, zlib + svb-zd (and the same reads uncompressed): four short reads, a truncated one, and 40 000 samples of two levels in
    turn — events like any read's, but a payload that deflates a hundredfold"""

    def __init__(self):
        rng = np.random.default_rng(1906)
        sigs = [levels_signal(n, rng) for n in (300, 451, 500, 0, 257, 600)]
        sigs[BIG] = np.tile(np.repeat(np.array([400, 600], dtype=np.int16), 10), 2000)
        self.intact = [record(i, s, ZS) for i, s in enumerate(sigs)]
        self.recs = list(self.intact)
        self.recs[BAD] = self.recs[BAD][: len(self.recs[BAD]) // 2]
        self.plain_intact = [record(i, s, (ob.REC_NONE, ob.SIG_NONE)) for i, s in enumerate(sigs)]
        self.plain = list(self.plain_intact)
        self.plain[BAD] = self.plain[BAD][: len(self.plain[BAD]) // 2]
        self.ref = np.clip(np.round(rng.normal(0.0, 32.0, 300)), -127, 127).astype(np.int16)

    def good(self, recs):
        return [recs[i] for i in GOOD]


@pytest.fixture(scope="module")
def batch():
    return Batch()


def test_the_batch_holds_what_the_test_is_about(batch):
    """asserted on the CPU, before any GPU test relies on it: the long record's payload is larger than the first guess of ANY record of the
    batch (4 x + 4 KiB of a zlib record: the decoders that keep no payload size one scratch slot for all), the truncated one does not inflate"""
    guess = [4 * len(r) + 4096 for r in batch.recs]
    assert len(zlib.decompress(batch.recs[BIG])) > max(guess) and len(batch.recs[BIG]) < 2000
    assert all(len(zlib.decompress(batch.recs[i])) <= guess[i] for i in GOOD if i != BIG)
    with pytest.raises(zlib.error):
        zlib.decompress(batch.recs[BAD])
    assert len(batch.recs) == 6 and len(batch.ref) == 300


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def _events(g, b, recs, methods, strict):
    rows, first, st = g.events.read_events(recs, *methods, raise_on_error=strict)
    return [rows[int(first[i]):int(first[i + 1])] for i in range(len(recs))], st, None


def _map(g, b, recs, methods, strict):
    rows, st = g.map.read_map(recs, b.ref, *methods, want_start=True, raise_on_error=strict, **KW)
    return [(rows[i], st[i]) for i in range(len(recs))], st, None


def _align(g, b, recs, methods, strict):
    rows, lo, hi, ev, st = g.align.read_align(recs, b.ref, *methods, raise_on_error=strict, **KW)
    return [(rows[i], lo[i], hi[i], ev[i], st[i]) for i in range(len(recs))], st, None


def _pileup(g, b, recs, methods, strict):
    with g.pileup.Pileup(b.ref, **KW) as h:
        rc, rows, st = h.add(recs, *methods, raise_on_error=strict)
        total, cols = h.close()
    assert rc == (ERR_DATA if len(recs) == 6 else 0)
    return [(rows[i], st[i]) for i in range(len(recs))], st, (total, cols)


def _diff(side):
    def run(g, b, recs, methods, strict):
        other = b.intact if len(recs) == 6 else b.good(b.intact)
        h = g.diff.Handle()
        try:
            rows, sa, sb = h.add(recs, methods, other, ZS, strict) if side == "a" else h.add(other, ZS, recs, methods, strict)
            acc = h.close()
        finally:
            h.abandon()
        st, clean = (sa, sb) if side == "a" else (sb, sa)
        assert not clean.any()
        return [rows[i] for i in range(len(recs))], st, acc
    return run


def _digest(via):
    def run(g, b, recs, methods, strict):
        out = g.digest.record_digests(recs, *methods, raise_on_error=strict, via=via)
        dg, st = out if not strict else (out, np.zeros(len(recs), dtype=np.int32))
        return [dg[i] for i in range(len(recs))], st, None
    return run


def _fstats(g, b, recs, methods, strict):
    h = g.fstats.Handle()
    try:
        st = h.add(recs, *methods, raise_on_error=strict)
        acc = h.close()
    finally:
        h.abandon()
    return [st[i] for i in range(len(recs))], st, acc


CALLS = {
    "s5gpu_signal_events_batch": (_events, ZS),
    "s5gpu_map_batch": (_map, ZS),
    "s5gpu_align_batch": (_align, ZS),
    "s5gpu_pileup_add_batch": (_pileup, ZS),
    "s5gpu_diff_add_batch-a": (_diff("a"), ZS),
    "s5gpu_diff_add_batch-b": (_diff("b"), ZS),
    "s5gpu_digest_batch": (_digest("batch"), ZS),
    "s5gpu_digest_stream": (_digest("stream"), ZS),
    "s5gpu_file_stats_add_stream": (_fstats, ZS),
    "s5gpu_file_stats_add_stream-plain": (_fstats, (ob.REC_NONE, ob.SIG_NONE)),   # the full decode of the chunk form
}


def _accumulated(name, got, want):
    """the accumulator after the six records against the one after the five good ones: one record more, and that one failed"""
    if name.startswith("s5gpu_pileup"):
        (gt, gc), (wt, wc) = got, want
        assert _same(gc, wc)
        for f in gt.dtype.names:
            assert _same(gt[f], wt[f] + 1 if f == "reads_skipped" else wt[f]), f
    elif name.startswith("s5gpu_diff"):
        for f in got.dtype.names:
            assert _same(got[f], want[f] + 1 if f in ("n_failed", "n_pairs") else want[f]), f
        assert got["n_failed"] == 1
    else:
        for f in got.dtype.names:
            assert _same(got[f], want[f] + 1 if f == "n_failed" else want[f]), f   # (n_reads: the reads that decoded)
        assert got["n_failed"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CALLS))
def test_a_corrupt_record_and_one_that_outgrows_its_slot_in_one_batch(gpu, batch, name):
    run, methods = CALLS[name]
    six = batch.recs if methods == ZS else batch.plain
    want, want_st, want_acc = run(gpu, batch, batch.good(six), methods, True)
    assert not want_st.any()                                               # (every good read decodes, has a query and a path)
    if not name.startswith("s5gpu_pileup"):                                # (Pileup.add hands the code back itself)
        with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
            run(gpu, batch, six, methods, True)
    assert gpu.L.s5gpu_set_option(b"no_such_option", 1) == -1              # a message of another call's in between
    got, st, acc = run(gpu, batch, six, methods, False)
    err = gpu.L.s5gpu_last_error().decode()
    print(name, "status", st.tolist(), "|", err)
    assert err.startswith(name.split("-")[0] + ":") and "corrupt" in err, err
    assert st[BAD] not in (0, 5, 6, 18, 19, 20)
    for k, i in enumerate(GOOD):
        assert st[i] == want_st[k], (i, st.tolist(), want_st.tolist())
        w, g_ = want[k], got[i]
        assert all(_same(x, y) for x, y in zip(g_, w)) if isinstance(w, tuple) else _same(g_, w), (name, i)
    if want_acc is not None:
        print(name, "accumulator", {f: acc[f].tolist() for f in acc.dtype.names if acc[f].ndim == 0} if not isinstance(acc, tuple) else acc[0])
        _accumulated(name, acc, want_acc)


@pytest.mark.gpu
def test_signal_stats_stream_decodes_once_so_the_outgrown_record_stays_undecoded(gpu, batch):
    """s5gpu_signal_stats_stream makes one decode and drops nothing.  The decode's own retry stops at the attempt that meets the corrupt
    record, which is the first: the four short reads have their statistics, the long one is left at status 5 with n = 0, as before the
    shared front existed."""
    want, wf = gpu.signals.signal_stats(batch.good(batch.recs), *ZS, quantiles=(0.5,), with_fields=True)
    assert not wf["status"].any() and want["n"].tolist() == [300, 451, 40000, 257, 600]
    with pytest.raises(gpu.lib.S5GpuError, match="rc=-5"):
        gpu.signals.signal_stats(batch.recs, *ZS, quantiles=(0.5,))
    assert gpu.L.s5gpu_set_option(b"no_such_option", 1) == -1
    got, f = gpu.signals.signal_stats(batch.recs, *ZS, quantiles=(0.5,), raise_on_error=False, with_fields=True)
    err = gpu.L.s5gpu_last_error().decode()
    print("s5gpu_signal_stats_stream status", f["status"].tolist(), "n", got["n"].tolist(), "|", err)
    assert err.startswith("s5gpu_signal_stats_stream:") and "corrupt" in err, err
    assert f["status"][BAD] not in (0, 5, 6) and got["n"][BAD] == 0
    assert f["status"][BIG] == 5 and got["n"][BIG] == 0
    for k, i in enumerate(GOOD):
        if i != BIG:
            assert f["status"][i] == 0 and got[i].tobytes() == want[k].tobytes(), i
