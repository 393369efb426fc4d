#!/usr/bin/env python3
"""What the level histograms and their comparison cost beside the table they stand next to (docs/codecs.md §4.23, k_pile_hist_accum and
k_pile_contrast).

  contrast_time.py [--reads 4096] [--rows 16384] [--ref 65536] [--narrow 512] [--reps 5] [--out FILE]

The two inputs are those of tools/pileup_long_time.py (spread over --ref columns, piled on --narrow), made by its `paths` with its seed.
For each, in ONE process, with the library's event hooks (s5gpu_event_*; median of --reps after 2 warm-ups):
  k_read_floor                     every byte the histogram call reads (queries, lo, hi, first, qlen, status) loaded once
  s5gpu_pileup_accum_long_dev      the table's call at its defaults on the same cells (events given), and its accumulate pass apart
  s5gpu_pile_hist_accum_long_dev   with pile_hist_cols 0, 64 and 256: the whole call, and its accumulate pass apart (pileup_long_passes 4)
and on the spread input's histogram (--ref columns) against the same cells shifted by one bin:
  k_read_floor                     the two histograms loaded once
  s5gpu_pile_contrast_dev          without tables
Every histogram is compared with the first of its input, and its columns' sums and cells with the table's n_events.  One JSON object per
line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib  # noqa: E402
from pileup_long_time import paths  # noqa: E402
from devtime import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--narrow", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    L.s5tool_read_floor_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q = a.reads, a.rows
    total = n * Q
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (total,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    wide = torch.randint(-127, 128, (a.ref,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    narrow = wide[:a.narrow].contiguous()
    ev = torch.zeros((total, 4), dtype=torch.int32, device="cuda")
    ev[:, 1] = torch.randint(4, 40, (total,), generator=g, device="cuda", dtype=torch.int32)
    first = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * Q).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    need = int(L.s5gpu_pileup_long_work_bytes(n, total))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = []
    kept = None

    def opt(key, v):
        _lib.check(L.s5gpu_set_option(key, v), key.decode())

    def floor_of(ins):
        def run():
            for t in ins:
                _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")
        return timed(L, run, a.reps)[0]

    for name, ref, advance in (("spread", wide, 0.75), ("piled", narrow, 400.0 / Q)):
        R = int(ref.numel())
        lo, hi = paths(n, Q, R, advance, g)
        cells = int((hi.to(torch.int64) - lo.to(torch.int64) + 1).sum().item())
        ins = [q, lo, hi, first, ql, st]
        floor_ms = floor_of(ins)
        acc = torch.zeros(int(L.s5gpu_pileup_bytes(R)), dtype=torch.uint8, device="cuda")
        hist = torch.zeros(int(L.s5gpu_pile_hist_bytes(R)), dtype=torch.uint8, device="cuda")

        def table():
            _lib.check(L.s5gpu_pileup_accum_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(),
                                                     st.data_ptr(), ev.data_ptr(), 0, work.data_ptr(), need, acc.data_ptr(), None), "s5gpu_pileup_accum_long_dev")

        def histo():
            _lib.check(L.s5gpu_pile_hist_accum_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, R, lo.data_ptr(), hi.data_ptr(), st.data_ptr(),
                                                        work.data_ptr(), need, hist.data_ptr(), None), "s5gpu_pile_hist_accum_long_dev")

        def parts(fn):
            ms, ms_min = timed(L, fn, a.reps)
            opt(b"pileup_long_passes", 4)                                   # (over the work area the whole call left)
            acc_ms = timed(L, fn, a.reps)[0]
            opt(b"pileup_long_passes", 7)
            return ms, ms_min, acc_ms

        _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
        t_ms, t_min, t_acc = parts(table)
        _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
        table()
        torch.cuda.synchronize()
        n_events = acc.cpu().numpy()[64:].view(_lib.PileCol)["n_events"].astype(np.int64)
        common = dict(input=name, reads=n, rows=Q, R=R, cells=cells, read_bytes=sum(t.numel() * t.element_size() for t in ins), read_floor_ms=round(floor_ms, 3))
        res.append(dict(kernel="k_pileup_long_* (the table, defaults, events given)", ms_median=round(t_ms, 3), ms_min=round(t_min, 3),
                        accumulate_ms=round(t_acc, 3), ns_per_cell=round(t_ms * 1e6 / cells, 4), **common))
        first_hist = None
        for cols in (0, 64, 256):
            opt(b"pile_hist_cols", cols)
            _lib.check(L.s5gpu_pile_hist_reset_dev(hist.data_ptr(), R, -128, 2, None), "reset")
            ms, ms_min, acc_ms = parts(histo)
            _lib.check(L.s5gpu_pile_hist_reset_dev(hist.data_ptr(), R, -128, 2, None), "reset")
            histo()
            torch.cuda.synchronize()
            raw = hist.cpu().numpy()
            head, counts = raw[:64].view(_lib.PileHistHead)[0], raw[64:].view("<u4").reshape(-1, 64)
            if first_hist is None:
                first_hist = raw.copy()
            res.append(dict(kernel="k_pile_hist_*", pile_hist_cols=cols, ms_median=round(ms, 3), ms_min=round(ms_min, 3), accumulate_ms=round(acc_ms, 3),
                            ns_per_cell=round(ms * 1e6 / cells, 4), accumulate_over_k_pileup_long_accum=round(acc_ms / t_acc, 3), call_over_table_call=round(ms / t_ms, 3),
                            over_read_floor=round(ms / floor_ms, 2), equals_first_hist=bool(np.array_equal(raw, first_hist)),
                            sums_equal_the_table=bool(np.array_equal(counts.sum(axis=1, dtype=np.int64), n_events) and int(head["cells"]) == cells), **common))
        opt(b"pile_hist_cols", 256)                                         # (the default)
        if name == "spread":
            kept = hist.clone()
        del lo, hi, acc, hist
    # the comparison: the spread histogram against its columns rolled by one bin
    R = a.ref
    other = kept.clone()
    other[64:] = torch.roll(kept[64:].view(R, 256), 4, 1).reshape(-1)
    rows = torch.zeros((R, 5), dtype=torch.int64, device="cuda")
    floor_ms = floor_of([kept, other])

    def contrast():
        _lib.check(L.s5gpu_pile_contrast_dev(kept.data_ptr(), other.data_ptr(), None, None, R, rows.data_ptr(), None), "s5gpu_pile_contrast_dev")
    ms, ms_min = timed(L, contrast, a.reps)
    torch.cuda.synchronize()
    h = rows.cpu().numpy().view(_lib.PileContrast).reshape(-1)
    res.append(dict(kernel="k_pile_contrast", R=R, ms_median=round(ms, 3), ms_min=round(ms_min, 3), read_bytes=int(2 * kept.numel()), read_floor_ms=round(floor_ms, 3),
                    over_read_floor=round(ms / floor_ms, 2), flags_seen=sorted(set(int(f) for f in h["flags"])), columns_with_a_gap=int((h["ks_num"] != 0).sum())))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
