#!/usr/bin/env python3
"""What refining an alignment costs beside the mapping and the path that it starts from (docs/codecs.md §4.20: k_path_fit, k_sdtw_win,
k_sdtw_trace_win).

  refine_time.py [--reads 65536] [--qlen 256] [--ref 65536] [--reps 5] [--out FILE]

Synthetic queries and a reference (uniform int16 in +-127, a fixed seed, those of sdtw_path_time.py) are made on the device; rows and paths
come from the library in the same run.  Then, in ONE process, with the library's event hooks (median of --reps after 2 warm-ups):
  s5gpu_sdtw_dev with want_start     the mapping that made the rows: reads x qlen x ref cells
  s5gpu_sdtw_path_dev                the path call on the same batch, the yardstick of the window call
  k_read_floor                       every byte k_path_fit reads (queries, lo, hi, qlen, status) loaded once (s5tool_read_floor_dev)
  s5gpu_path_fit_dev                 k_path_fit, with queries_out
  s5gpu_sdtw_window_dev              pad 0 and pad 16
  s5gpu_refine_dev                   2 rounds, with the default parameters and with parameters that accept every fit (so that every read
                                     runs both rounds)
One JSON object per line; --out also writes them to a file."""
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


def counts(t):
    return {str(int(k)): int(v) for k, v in zip(*np.unique(t.cpu().numpy(), return_counts=True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--qlen", type=int, default=256)
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    L.s5tool_read_floor_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q, R = a.reads, a.qlen, a.ref
    wmax = 4 * Q + 32
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (n, Q), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    ref = torch.randint(-127, 128, (R,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()

    def i32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda")
    rows, lo, hi, st = i32(n, 4), i32(n, Q), i32(n, Q), i32(n)
    rows2, lo2, hi2, st2, rounds = i32(n, 4), i32(n, Q), i32(n, Q), i32(n), i32(n)
    q2 = torch.zeros((n, Q), dtype=torch.int16, device="cuda")
    fit = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    slot = int(L.s5gpu_sdtw_path_slot_bytes(Q, wmax))
    scratch = torch.empty(slot * n // 4 + 4, dtype=torch.int32, device="cuda")
    wb = int(L.s5gpu_refine_work_bytes(n, Q))
    work = torch.empty(wb // 8 + 2, dtype=torch.int64, device="cuda")
    sink = i32(4)
    defaults = _lib.RefineParams(0.5, 2.0, 64.0, 127, 16, 16, 2)
    every = _lib.RefineParams(1e-6, 1e6, 1e9, 127, 16, 2, 2)
    res = []

    def sdtw():
        _lib.check(L.s5gpu_sdtw_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, 1, rows.data_ptr(), None), "s5gpu_sdtw_dev")

    def path():
        _lib.check(L.s5gpu_sdtw_path_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, rows.data_ptr(), wmax, scratch.data_ptr(), slot * n, lo.data_ptr(),
                                         hi.data_ptr(), st.data_ptr(), None), "s5gpu_sdtw_path_dev")

    def floor():
        for t in (q, lo, hi, ql, st):
            _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")

    def fit_call():
        _lib.check(L.s5gpu_path_fit_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(), st.data_ptr(), wmax, C.byref(defaults),
                                        fit.data_ptr(), q2.data_ptr(), st2.data_ptr(), None), "s5gpu_path_fit_dev")

    def window(pad):
        _lib.check(L.s5gpu_sdtw_window_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, rows.data_ptr(), pad, wmax, scratch.data_ptr(), slot * n,
                                           rows2.data_ptr(), lo2.data_ptr(), hi2.data_ptr(), st2.data_ptr(), None), "s5gpu_sdtw_window_dev")

    def refine(p):
        _lib.check(L.s5gpu_refine_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(), st.data_ptr(), wmax,
                                      C.byref(p), scratch.data_ptr(), slot * n, work.data_ptr(), wb, q2.data_ptr(), rows2.data_ptr(), lo2.data_ptr(), hi2.data_ptr(),
                                      fit.data_ptr(), st2.data_ptr(), rounds.data_ptr(), None), "s5gpu_refine_dev")

    map_ms, map_min = timed(L, sdtw, a.reps)
    res.append(dict(kernel="s5gpu_sdtw_dev (k_sdtw, want_start)", reads=n, qlen=Q, R=R, cells=n * Q * R, ms_median=round(map_ms, 3), ms_min=round(map_min, 3)))
    path_ms, path_min = timed(L, path, a.reps)
    torch.cuda.synchronize()
    h = rows.cpu().numpy()
    span = (h[:, 3] - h[:, 2] + 1).astype(np.int64)
    res.append(dict(kernel="s5gpu_sdtw_path_dev", wmax=wmax, slot_bytes=slot, ms_median=round(path_ms, 3), ms_min=round(path_min, 3), span_mean=round(float(span.mean()), 1),
                    window_cells=int((span * Q).sum()), status_counts=counts(st)))
    floor_ms, floor_min = timed(L, floor, a.reps)
    read_bytes = sum(t.numel() * t.element_size() for t in (q, lo, hi, ql, st))
    res.append(dict(kernel="k_read_floor (16-byte loads) over what k_path_fit reads", bytes=read_bytes, ms_median=round(floor_ms, 3), ms_min=round(floor_min, 3),
                    gb_per_s=round(read_bytes / floor_ms / 1e6, 1)))
    ms, ms_min = timed(L, fit_call, a.reps)
    torch.cuda.synchronize()
    cells = int(fit.cpu().numpy()[:, 2].sum())
    res.append(dict(kernel="s5gpu_path_fit_dev (k_path_fit)", ms_median=round(ms, 3), ms_min=round(ms_min, 3), cells=cells, over_read_floor=round(ms / floor_ms, 2),
                    over_path_call=round(ms / path_ms, 3), status_counts=counts(st2)))
    for pad in (0, 16):
        ms, ms_min = timed(L, lambda: window(pad), a.reps)
        torch.cuda.synchronize()
        h2 = rows2.cpu().numpy()
        wcells = int(((np.minimum(R - 1, h[:, 3] + pad) - np.maximum(0, h[:, 2] - pad) + 1).astype(np.int64) * Q).sum())
        res.append(dict(kernel="s5gpu_sdtw_window_dev (k_sdtw_win, k_sdtw_trace_win)", pad=pad, ms_median=round(ms, 3), ms_min=round(ms_min, 3), window_cells=wcells,
                        over_path_call=round(ms / path_ms, 3), status_counts=counts(st2),
                        equals_the_path_call=bool(pad == 0 and np.array_equal(h2, h) and torch.equal(lo2, lo) and torch.equal(hi2, hi)) if pad == 0 else None,
                        cost_not_above_first=bool((h2[:, 0].astype(np.int64) <= h[:, 0].astype(np.int64)).all())))
    for name, p in (("defaults", defaults), ("every fit accepted", every)):
        ms, ms_min = timed(L, lambda: refine(p), a.reps)
        torch.cuda.synchronize()
        h2, ok = rows2.cpu().numpy(), (st2.cpu().numpy() == 0)
        res.append(dict(kernel="s5gpu_refine_dev, 2 rounds", parameters=name, ms_median=round(ms, 3), ms_min=round(ms_min, 3), over_mapping=round(ms / map_ms, 4),
                        over_path_call=round(ms / path_ms, 3), status_counts=counts(st2), rounds_counts=counts(rounds),
                        cost_first_mean=round(float(h[ok, 0].mean()), 1) if ok.any() else None, cost_refined_mean=round(float(h2[ok, 0].mean()), 1) if ok.any() else None))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
