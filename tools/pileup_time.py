#!/usr/bin/env python3
"""What the per-position table costs beside the paths it transposes, and what the LDS window buys (docs/codecs.md §4.18, k_pileup).

  pileup_time.py [--reads 65536] [--qlen 256] [--ref 65536] [--narrow 512] [--reps 5] [--out FILE]

The synthetic queries and reference of tools/sdtw_path_time.py (uniform int16 in +-127, a fixed seed) are made on the device; the rows and
paths come from the library in the same run.  Two inputs:
  spread        the paths as they fall on the reference of --ref levels
  concentrated  the same queries against a reference of --narrow levels: every read piles on the same columns (target enrichment)
For each, in ONE process, with the library's event hooks (s5gpu_event_*; median of --reps after 2 warm-ups):
  s5gpu_sdtw_path_dev       the call whose output is transposed: the yardstick
  k_read_floor              every byte k_pileup reads (queries, lo, hi, events, qlen, status) loaded once
  s5gpu_pileup_accum_dev    with pileup_lds_cols at 0 (every cell a global atomic), 256 and 1024, events given
Every table is compared with the first of its input (the result must not depend on the window), and its cost with the sum of the rows' costs.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--qlen", type=int, default=256)
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--narrow", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    L.s5tool_read_floor_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q = a.reads, a.qlen
    wmax = 4 * Q
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (n, Q), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    wide = torch.randint(-127, 128, (a.ref,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    narrow = wide[:a.narrow].contiguous()
    ev = torch.zeros((n, Q, 4), dtype=torch.int32, device="cuda")
    ev[:, :, 1] = torch.randint(4, 40, (n, Q), generator=g, device="cuda", dtype=torch.int32)
    rows = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    lo = torch.zeros((n, Q), dtype=torch.int32, device="cuda")
    hi = torch.zeros((n, Q), dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    slot = int(L.s5gpu_sdtw_path_slot_bytes(Q, wmax))
    scratch = torch.empty(slot * n // 4 + 4, dtype=torch.int32, device="cuda")
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = []
    for name, ref in (("spread", wide), ("concentrated", narrow)):
        R = int(ref.numel())
        _lib.check(L.s5gpu_sdtw_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, 1, rows.data_ptr(), None), "s5gpu_sdtw_dev")

        def path():
            _lib.check(L.s5gpu_sdtw_path_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, rows.data_ptr(), wmax, scratch.data_ptr(), slot * n,
                                             lo.data_ptr(), hi.data_ptr(), st.data_ptr(), None), "s5gpu_sdtw_path_dev")

        def floor():
            for t in (q, lo, hi, ev, ql, st):
                _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")

        path_ms, path_min = timed(L, path, a.reps)
        floor_ms, floor_min = timed(L, floor, a.reps)
        torch.cuda.synchronize()
        h_rows, h_st, h_lo, h_hi = rows.cpu().numpy(), st.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
        ok = h_st == 0
        cells = int((h_hi[ok] - h_lo[ok] + 1).sum())
        read_bytes = sum(t.numel() * t.element_size() for t in (q, lo, hi, ev, ql, st))
        common = dict(input=name, reads=n, qlen=Q, R=R, reads_with_a_path=int(ok.sum()), cells=cells, columns_touched=0,
                      path_call_ms=round(path_ms, 3), read_bytes=read_bytes, read_floor_ms=round(floor_ms, 3))
        nb = int(L.s5gpu_pileup_bytes(R))
        acc = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        first = None
        for cols in (0, 256, 1024):
            _lib.check(L.s5gpu_set_option(b"pileup_lds_cols", cols), "opt")

            def pile():
                _lib.check(L.s5gpu_pileup_accum_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(), st.data_ptr(),
                                                    ev.data_ptr(), acc.data_ptr(), None), "s5gpu_pileup_accum_dev")

            _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
            ms, ms_min = timed(L, pile, a.reps)
            _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")
            pile()
            torch.cuda.synchronize()
            h = acc.cpu().numpy()
            total = h[:64].view(_lib.PileTotal)[0]
            if first is None:
                first = h.copy()
            common["columns_touched"] = int((h[64:].view(_lib.PileCol)["n_events"] != 0).sum())
            res.append(dict(kernel="k_pileup", pileup_lds_cols=cols, ms_median=round(ms, 3), ms_min=round(ms_min, 3), gcells_per_s=round(cells / ms / 1e6, 2),
                            over_path_call=round(ms / path_ms, 3), over_read_floor=round(ms / floor_ms, 2),
                            equals_first_table=bool(np.array_equal(h, first)),
                            cost_is_sum_of_rows=bool(int(total["cost"]) == int(h_rows[ok, 0].astype(np.int64).sum()) and int(total["cells"]) == cells
                                                     and int(total["reads_used"]) == int(ok.sum())), **common))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
