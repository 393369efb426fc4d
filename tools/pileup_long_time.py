#!/usr/bin/env python3
"""What the whole-read pileup costs beside the fixed-pitch kernel it extends (docs/codecs.md §4.22, k_pileup_long_*).

  pileup_long_time.py [--reads 4096] [--rows 16384] [--ref 65536] [--narrow 512] [--reps 5] [--no-events] [--out FILE]

The workload has the shape of tools/extend_time.py: --reads reads of --rows rows each.  The paths are not DTW's: random valid monotone paths
made on the device with a fixed seed (the kernels only see lo and hi).  Two inputs:
  spread   every read walks about three quarters of its rows in columns of a reference of --ref levels, from a random start
  piled    every read walks about 400 columns of a reference of --narrow levels: all reads pile on the same columns
For each, in ONE process, with the library's event hooks (s5gpu_event_*; median of --reps after 2 warm-ups):
  k_read_floor                  every byte the ragged call reads (queries, lo, hi, events, first, qlen, status) loaded once
  s5gpu_pileup_accum_dev        the fixed-pitch kernel on the same cells cut into 1024-row matrix reads, at its defaults: the yardstick
  s5gpu_pileup_accum_long_dev   with pileup_long_sort 0 and 1 and pileup_long_cols 0 and 1024: the whole call, and its plan, check (with the
                                sort) and accumulate passes apart (pileup_long_passes)
Every ragged table is compared with the first of its input, and its n_events, sums and cells with the fixed-pitch table's (depth differs: a
cut read counts once per piece).  One JSON object per line; --out also writes them to a file."""
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
from devtime import timed  # noqa: E402


def paths(n, Q, R, advance, g):
    """lo, hi [n * Q] int32: per row a step of 0 or 1 and a span of 1 or 2, `advance` columns a row on average, clamped to R - 1"""
    lo = torch.empty(n * Q, dtype=torch.int32, device="cuda")
    hi = torch.empty(n * Q, dtype=torch.int32, device="cuda")
    room = max(R - int(Q * advance * 1.2), 1)
    for b in range(0, n, 256):
        m = min(256, n - b)
        step = (torch.rand((m, Q), generator=g, device="cuda") < advance * 2 / 3).to(torch.int64)
        span = (torch.rand((m, Q), generator=g, device="cuda") < advance / 3).to(torch.int64)          # span - 1
        step[:, 0] = 0
        start = torch.randint(0, room, (m, 1), generator=g, device="cuda", dtype=torch.int64)
        h = start + torch.cumsum(step + span, 1)
        l = h - span
        lo[b * Q:(b + m) * Q] = l.clamp_(max=R - 1).to(torch.int32).reshape(-1)
        hi[b * Q:(b + m) * Q] = h.clamp_(max=R - 1).to(torch.int32).reshape(-1)
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--narrow", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-events", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.rows % 1024 == 0
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
    ev = None
    if not a.no_events:
        ev = torch.zeros((total, 4), dtype=torch.int32, device="cuda")
        ev[:, 1] = torch.randint(4, 40, (total,), generator=g, device="cuda", dtype=torch.int32)
    first = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * Q).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    ql_cut = torch.full((total // 1024,), 1024, dtype=torch.int32, device="cuda")
    st_cut = torch.zeros(total // 1024, dtype=torch.int32, device="cuda")
    need = int(L.s5gpu_pileup_long_work_bytes(n, total))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    evp = ev.data_ptr() if ev is not None else None
    res = []

    def opt(key, v):
        _lib.check(L.s5gpu_set_option(key, v), key.decode())

    for name, ref, advance in (("spread", wide, 0.75), ("piled", narrow, 400.0 / Q)):
        R = int(ref.numel())
        lo, hi = paths(n, Q, R, advance, g)
        cells = int((hi.to(torch.int64) - lo.to(torch.int64) + 1).sum().item())
        ins = [t for t in (q, lo, hi, ev, first, ql, st) if t is not None]

        def floor():
            for t in ins:
                _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")

        floor_ms, _ = timed(L, floor, a.reps)
        acc = torch.zeros(int(L.s5gpu_pileup_bytes(R)), dtype=torch.uint8, device="cuda")

        def table(fn):
            _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
            fn()
            torch.cuda.synchronize()
            h = acc.cpu().numpy()
            return h[:64].view(_lib.PileTotal)[0].copy(), h[64:].view(_lib.PileCol).copy(), h.copy()

        def fixed():
            _lib.check(L.s5gpu_pileup_accum_dev(total // 1024, q.data_ptr(), 1024, ql_cut.data_ptr(), ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(),
                                                st_cut.data_ptr(), evp, acc.data_ptr(), None), "s5gpu_pileup_accum_dev")

        def ragged():
            _lib.check(L.s5gpu_pileup_accum_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(),
                                                     st.data_ptr(), evp, 0, work.data_ptr(), need, acc.data_ptr(), None), "s5gpu_pileup_accum_long_dev")

        _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
        fixed_ms, fixed_min = timed(L, fixed, a.reps)
        ft, fc, _ = table(fixed)
        common = dict(input=name, reads=n, rows=Q, R=R, cells=cells, columns_touched=int((fc["n_events"] != 0).sum()), events=ev is not None,
                      read_bytes=sum(t.numel() * t.element_size() for t in ins), read_floor_ms=round(floor_ms, 3))
        res.append(dict(kernel="k_pileup on 1024-row pieces", ms_median=round(fixed_ms, 3), ms_min=round(fixed_min, 3), ns_per_cell=round(fixed_ms * 1e6 / cells, 4),
                        cells_ok=bool(int(ft["cells"]) == cells), **common))
        first_table = None
        for sort in (0, 1):
            for cols in (0, 1024):
                opt(b"pileup_long_sort", sort)
                opt(b"pileup_long_cols", cols)
                _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
                ms, ms_min = timed(L, ragged, a.reps)
                parts = {}
                for key, bits in (("plan_ms", 1), ("check_and_sort_ms", 2), ("accumulate_ms", 4)):   # (over the work area the whole call left)
                    opt(b"pileup_long_passes", bits)
                    parts[key] = round(timed(L, ragged, a.reps)[0], 3)
                opt(b"pileup_long_passes", 7)
                t, c, raw = table(ragged)
                if first_table is None:
                    first_table = raw
                same = all(np.array_equal(c[k], fc[k]) for k in ("n_events", "n_samples", "sum_q", "sumsq_q", "sum_cost", "min_q", "max_q"))
                res.append(dict(kernel="k_pileup_long_*", pileup_long_sort=sort, pileup_long_cols=cols, ms_median=round(ms, 3), ms_min=round(ms_min, 3),
                                ns_per_cell=round(ms * 1e6 / cells, 4), per_cell_over_k_pileup=round(ms / fixed_ms, 3), over_read_floor=round(ms / floor_ms, 2),
                                equals_first_table=bool(np.array_equal(raw, first_table)), sums_equal_k_pileup=bool(same and int(t["cells"]) == cells and
                                                                                                                     int(t["cost"]) == int(ft["cost"])),
                                reads_used=int(t["reads_used"]), **parts, **common))
        opt(b"pileup_long_sort", 1)                                        # (the defaults)
        opt(b"pileup_long_cols", 1024)
        del lo, hi, acc
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
