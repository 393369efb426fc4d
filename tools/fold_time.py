#!/usr/bin/env python3
"""What the fold of a table and of a level histogram onto k-mers costs beside a plain read of its inputs (docs/codecs.md §4.26, k_pile_fold
and k_pile_hist_fold).

  fold_time.py [--cols 4194304] [--reps 5] [--out FILE]

--cols columns (default 2^22) with random non-empty content.  In ONE process, with the library's event hooks (s5gpu_event_*; median of
--reps after 2 warm-ups), for classes uniform over K = 4^5, 4^6 and 4^9 and for all columns in one class (the worst contention):
  k_read_floor              every byte the call reads loaded once: 52 bytes a column for the table (48 and the class), 260 for the histogram
  s5gpu_pileup_fold_dev     at K = 4^5 with pile_fold_lds 0 and 1 (above 1024 classes the option does not count)
  s5gpu_pile_hist_fold_dev
Every output is checked: its cells are the input's, and at K = 4^5 the two values of pile_fold_lds give the same bytes.  One JSON object
per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, contrast, pileup  # noqa: E402
from devtime import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    L.s5tool_read_floor_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    R = a.cols
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5106)

    def rnd(lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=g, device="cuda", dtype=torch.int64)
    # the table: 8 words of head, 6 a column (depth | n_events << 32, n_samples, sum_q, sumsq_q, sum_cost, min_q | max_q << 32)
    n_events = rnd(1, 40, (R,))
    table = torch.zeros(8 + 6 * R, dtype=torch.int64, device="cuda")
    body = table[8:].view(R, 6)
    body[:, 0] = rnd(1, 3, (R,)).minimum(n_events) | (n_events << 32)
    body[:, 1] = n_events * rnd(4, 40, (R,))
    body[:, 2] = n_events * rnd(-100, 100, (R,))
    body[:, 3] = n_events * rnd(0, 10000, (R,))
    body[:, 4] = n_events * rnd(0, 50, (R,))
    body[:, 5] = (rnd(-127, 0, (R,)) & 0xFFFFFFFF) | (rnd(0, 128, (R,)) << 32)
    cells = int(n_events.sum().item())
    table[0], table[3], table[4], table[5] = 1000, cells, int(body[:, 4].sum().item()), R
    acc_in = table.view(torch.uint8)
    # the histogram: 16 words of head, 64 a column; the bins of a column add up to anything: it is timed, not compared with the table
    hist32 = torch.zeros(16 + 64 * R, dtype=torch.int32, device="cuda")
    hist32[16:] = torch.randint(0, 3, (64 * R,), generator=g, device="cuda", dtype=torch.int32)
    hcells = int(hist32[16:].sum(dtype=torch.int64).item())
    assert hcells < (1 << 31)                                              # (one 32-bit word of the head's 64-bit cells)
    hist32[0], hist32[2],hist32[8], hist32[9], hist32[10], hist32[11] = hcells, 1000, R, -128, 2, 64
    hist_in = hist32.view(torch.uint8)
    sink = torch.zeros(4, dtype=torch.int32, device="cuda")
    res = []

    def opt(key, v):
        _lib.check(L.s5gpu_set_option(key, v), key.decode())

    def floor_of(ins):
        def run():
            for t in ins:
                _lib.check(L.s5tool_read_floor_dev(t.data_ptr(), t.numel() * t.element_size(), sink.data_ptr(), None), "s5tool_read_floor_dev")
        return timed(L, run, a.reps)[0]

    for name, K in (("uniform", 4 ** 5), ("uniform", 4 ** 6), ("uniform", 4 ** 9), ("one class", 4 ** 5)):
        cls = (rnd(0, K, (R,)) if name == "uniform" else torch.full((R,), 7, dtype=torch.int64, device="cuda")).to(torch.int32).contiguous()
        t_floor, h_floor = floor_of([acc_in, cls]), floor_of([hist_in, cls])
        first = None
        for lds in (0, 1) if K <= 1024 else (1,):
            opt(b"pile_fold_lds", lds)
            out = pileup.new_acc(K)

            def fold():
                _lib.check(L.s5gpu_pileup_fold_dev(acc_in.data_ptr(), R, cls.data_ptr(), K, out.data_ptr(), None), "s5gpu_pileup_fold_dev")
            ms, ms_min = timed(L, fold, a.reps)
            out = pileup.new_acc(K)
            fold()
            total, cols = pileup.to_host(out)
            raw = out.cpu().numpy()
            first = raw if first is None else first
            res.append(dict(kernel="k_pile_fold", classes=name, K=K, R=R, pile_fold_lds=lds if K <= 1024 else None, ms_median=round(ms, 3), ms_min=round(ms_min, 3),
                            read_bytes=52 * R, read_floor_ms=round(t_floor, 3), over_read_floor=round(ms / t_floor, 2), GBps=round(52 * R / ms / 1e6, 1),
                            cells_kept=bool(int(total["cells"]) == cells == int(cols["n_events"].astype(np.int64).sum())), equals_first=bool(np.array_equal(raw, first))))
        hout = contrast.new_hist(K)

        def hfold():
            _lib.check(L.s5gpu_pile_hist_fold_dev(hist_in.data_ptr(), R, cls.data_ptr(), K, hout.data_ptr(), None), "s5gpu_pile_hist_fold_dev")
        ms, ms_min = timed(L, hfold, a.reps)
        hout = contrast.new_hist(K)
        hfold()
        head, counts = contrast.hist_to_host(hout)
        res.append(dict(kernel="k_pile_hist_fold", classes=name, K=K, R=R, ms_median=round(ms, 3), ms_min=round(ms_min, 3), read_bytes=260 * R, read_floor_ms=round(h_floor, 3),
                        over_read_floor=round(ms / h_floor, 2), GBps=round(260 * R / ms / 1e6, 1),
                        cells_kept=bool(int(head["cells"]) == hcells == int(counts.sum(dtype=np.int64)))))
        del cls
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
