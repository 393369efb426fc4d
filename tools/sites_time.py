#!/usr/bin/env python3
"""What the read x site matrix and its scores cost beside the level histogram they are held against (docs/codecs.md §4.25, k_site_cells and
k_site_score).

  sites_time.py [--reads 4096] [--rows 16384] [--ref 65536] [--narrow 512] [--reps 5] [--out FILE]

The two inputs are those of tools/pileup_long_time.py (spread over --ref columns, piled on --narrow), made by its `paths` with its seed.
For each, in ONE process, with the library's event hooks (s5gpu_event_*; median of --reps after 2 warm-ups):
  k_read_floor                     every byte the call reads (queries, lo, hi, first, qlen, status) loaded once
  the plan and the check           alone (site_passes 2)
  s5gpu_pile_hist_accum_long_dev   at its shipped window: the whole call, and k_pile_hist_accum apart (pileup_long_passes 4): the yardstick
  s5gpu_site_cells_long_dev        at M = 16, M = 1024 and every covered column up to the cap of 2^27 entries, the sites spread evenly over the
                                   columns the reads cover: the whole call, and the fill and k_site_cells apart (site_passes 1 and 4)
and on the spread input at M = 1024:
  k_read_floor                     the matrix loaded once
  s5gpu_site_score_dev             against the input's own histogram
After the timings every matrix is made once more and its sites' cells are compared with the histogram's columns.  One JSON object per line;
--out also writes them to a file."""
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

ENTRIES_MAX = 1 << 27


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
    first = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * Q).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    need = int(L.s5gpu_pileup_long_work_bytes(n, total))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = []

    def opt(key, v):
        _lib.check(L.s5gpu_set_option(key, v), key.decode())

    def floor_of(ins):
        def run():
            for t in ins:
                _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")
        return timed(L, run, a.reps)[0]

    for name, R, advance in (("spread", a.ref, 0.75), ("piled", a.narrow, 400.0 / Q)):
        lo, hi = paths(n, Q, R, advance, g)
        cells = int((hi.to(torch.int64) - lo.to(torch.int64) + 1).sum().item())
        c0, c1 = int(lo.min().item()), int(hi.max().item())
        ins = [q, lo, hi, first, ql, st]
        floor_ms = floor_of(ins)
        hist = torch.zeros(int(L.s5gpu_pile_hist_bytes(R)), dtype=torch.uint8, device="cuda")
        common = dict(input=name, reads=n, rows=Q, R=R, cells=cells, covered=[c0, c1], read_bytes=sum(t.numel() * t.element_size() for t in ins),
                      read_floor_ms=round(floor_ms, 3))

        def histo():
            _lib.check(L.s5gpu_pile_hist_accum_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, R, lo.data_ptr(), hi.data_ptr(), st.data_ptr(),
                                                        work.data_ptr(), need, hist.data_ptr(), None), "s5gpu_pile_hist_accum_long_dev")
        _lib.check(L.s5gpu_pile_hist_reset_dev(hist.data_ptr(), R, -128, 2, None), "reset")
        h_ms, h_min = timed(L, histo, a.reps)
        opt(b"pileup_long_passes", 4)                                       # (over the work area the whole call left)
        h_acc = timed(L, histo, a.reps)[0]
        opt(b"pileup_long_passes", 7)
        _lib.check(L.s5gpu_pile_hist_reset_dev(hist.data_ptr(), R, -128, 2, None), "reset")
        histo()
        torch.cuda.synchronize()
        col_cells = hist.cpu().numpy()[64:].view("<u4").reshape(-1, 64).sum(axis=1, dtype=np.int64)
        res.append(dict(kernel="k_pile_hist_* (the yardstick, pile_hist_cols 256)", ms_median=round(h_ms, 3), ms_min=round(h_min, 3), k_pile_hist_accum_ms=round(h_acc, 3),
                        over_read_floor=round(h_ms / floor_ms, 2), **common))
        plan_ms, seen = None, set()
        for want_m in (16, 1024, min(ENTRIES_MAX // n, 1 << 16)):
            M = min(want_m, c1 - c0 + 1)
            sites_h = np.unique(np.linspace(c0, c1, M).astype(np.int64)).astype(np.uint32)
            M = len(sites_h)
            if M in seen:                                                   # (the piled input covers fewer columns than 1024)
                continue
            seen.add(M)
            sites = torch.from_numpy(sites_h.view(np.int32)).to("cuda")
            out = torch.empty((M, n, 2), dtype=torch.int64, device="cuda")

            def cells_call():
                _lib.check(L.s5gpu_site_cells_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, R, lo.data_ptr(), hi.data_ptr(), st.data_ptr(),
                                                       sites.data_ptr(), M, work.data_ptr(), need, out.data_ptr(), None, None), "s5gpu_site_cells_long_dev")
            ms, ms_min = timed(L, cells_call, a.reps)
            part = {}
            for label, passes in (("k_site_fill_ms", 1), ("plan_check_ms", 2), ("k_site_cells_ms", 4)):   # (over the work area the whole call left)
                opt(b"site_passes", passes)
                part[label] = round(timed(L, cells_call, a.reps)[0], 3)
            opt(b"site_passes", 7)
            plan_ms = part["plan_check_ms"]
            cells_call()
            torch.cuda.synchronize()
            got = out[:, :, 1].bitwise_and(0xFFFFFFFF).sum(dim=1).cpu().numpy()     # SITE_CELL.cells: the low word of the second
            res.append(dict(kernel="k_site_*", M=M, ms_median=round(ms, 3), ms_min=round(ms_min, 3), matrix_bytes=16 * M * n,
                            k_site_cells_over_k_pile_hist_accum=round(part["k_site_cells_ms"] / h_acc, 3), call_over_hist_call=round(ms / h_ms, 3),
                            over_read_floor=round(ms / floor_ms, 2), hits=int(got.sum()), cells_equal_the_histogram=bool(np.array_equal(got, col_cells[sites_h])),
                            **part, **common))
            if name == "spread" and want_m == 1024:
                rows = torch.empty((M, n, 2), dtype=torch.int64, device="cuda")
                s_floor = floor_of([out])

                def score():
                    _lib.check(L.s5gpu_site_score_dev(out.data_ptr(), n, sites.data_ptr(), M, hist.data_ptr(), R, rows.data_ptr(), None), "s5gpu_site_score_dev")
                s_ms, s_min = timed(L, score, a.reps)
                torch.cuda.synchronize()
                r = rows.cpu().numpy().view(_lib.SiteScore).reshape(M, n)
                res.append(dict(kernel="k_site_score", M=M, reads=n, ms_median=round(s_ms, 3), ms_min=round(s_min, 3), read_bytes=16 * M * n, write_bytes=16 * M * n,
                                read_floor_ms=round(s_floor, 3), over_read_floor=round(s_ms / s_floor, 2), flags_seen=sorted(set(int(f) for f in np.unique(r["flags"]))),
                                rows_with_a_cell=int((r["flags"] & 1 == 0).sum())))
                del rows
            del out, sites
        res.append(dict(kernel="k_pileup_long_plan + k_pileup_long_check (no sort)", ms_median=plan_ms, **common))
        del lo, hi, hist
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
