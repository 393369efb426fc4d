#!/usr/bin/env python3
"""What subsequence DTW costs per cell (docs/codecs.md §4.16, k_sdtw).

  sdtw_time.py [--reads 65536] [--qlen 256] [--refs 4096,65536] [--reps 5] [--out FILE]

Synthetic queries and references (uniform int16 in +-127, a fixed seed) are made on the device; then, in ONE process, s5gpu_sdtw_dev is timed
with the library's event hooks (s5gpu_event_*; median of --reps launches after 2 warm-ups) for every reference length, without and with
want_start.  A call is one launch per lane height that the pitch allows (--qlen 256: G = 1, 2, 4; the waves of the first two return at once),
so the time is that of k_sdtw<4> and two empty grids.  Cells are reads x qlen x R.  The two variants' cost and end columns are compared.
One JSON object per line; --out also writes them to a file."""
import argparse
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
    ap.add_argument("--refs", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q = a.reads, a.qlen
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (n, Q), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    out = {ws: torch.zeros((n, 4), dtype=torch.int32, device="cuda") for ws in (0, 1)}
    lane_height = next(h for h in (1, 2, 4, 8, 16) if 64 * h >= Q)
    res = []
    for R in [int(v) for v in a.refs.split(",")]:
        ref = torch.randint(-127, 128, (R,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
        cells = n * Q * R
        for ws in (0, 1):
            def run():
                _lib.check(L.s5gpu_sdtw_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, ws, out[ws].data_ptr(), None), "s5gpu_sdtw_dev")
            ms, ms_min = timed(L, run, a.reps)
            res.append(dict(kernel="k_sdtw<%d, %s>" % (lane_height, "true" if ws else "false"), reads=n, qlen=Q, R=R, want_start=bool(ws), cells=cells,
                            ms_median=round(ms, 3), ms_min=round(ms_min, 3), gcells_per_s=round(cells / ms / 1e6, 1)))
        torch.cuda.synchronize()
        same = bool(torch.equal(out[0][:, [0, 1, 3]], out[1][:, [0, 1, 3]])) and bool((out[0][:, 2] == -1).all().item()) and bool((out[1][:, 2] >= 0).all().item())
        res[-1]["cost_and_end_equal_without_start"] = same
        res[-1]["mean_cost_per_event"] = round(float(out[1][:, 0].to(torch.float64).mean().item()) / Q, 3)
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
