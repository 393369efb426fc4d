#!/usr/bin/env python3
"""What the second-best hit costs beside the best one (docs/codecs.md §4.19, k_sdtw2 against k_sdtw).

  sdtw2_time.py [--reads 65536] [--qlen 256] [--refs 4096,65536] [--reps 5] [--block-shift B] [--out FILE]

The workload of tools/sdtw_time.py: synthetic queries and references (uniform int16 in +-127, a fixed seed) made on the device; in ONE
process s5gpu_sdtw_dev and s5gpu_sdtw2_dev are timed one after the other with the library's event hooks (median of --reps launches after 2
warm-ups) for every reference length, without and with want_start.  The rows of the two calls are compared bit for bit, and the second rows
are summarised (reads with a runner-up, mean mapq).  --block-shift: default the smallest block that holds --qlen columns.
One JSON object per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from slow5tools_amd import _lib  # noqa: E402
from slow5tools_amd import map as smap  # noqa: E402
from tools.devtime import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=65536)
    ap.add_argument("--qlen", type=int, default=256)
    ap.add_argument("--refs", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block-shift", type=int)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q = a.reads, a.qlen
    bshift = smap.default_bshift(Q) if a.block_shift is None else a.block_shift
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (n, Q), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    old, new, sec = (torch.zeros((n, 4), dtype=torch.int32, device="cuda") for _ in range(3))
    lane_height = next(h for h in (1, 2, 4, 8, 16) if 64 * h >= Q)
    res = []
    for R in [int(v) for v in a.refs.split(",")]:
        ref = torch.randint(-127, 128, (R,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
        cells = n * Q * R
        for ws in (0, 1):
            def run_old():
                _lib.check(L.s5gpu_sdtw_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, ws, old.data_ptr(), None), "s5gpu_sdtw_dev")

            def run_new():
                _lib.check(L.s5gpu_sdtw2_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, ws, bshift, new.data_ptr(), sec.data_ptr(), None),
                           "s5gpu_sdtw2_dev")
            ms_old, min_old = timed(L, run_old, a.reps)
            ms_new, min_new = timed(L, run_new, a.reps)
            torch.cuda.synchronize()
            res.append(dict(kernels="k_sdtw<%d, %s> | k_sdtw2" % (lane_height, "true" if ws else "false"), reads=n, qlen=Q, R=R, want_start=bool(ws),
                            block_shift=bshift, cells=cells, sdtw_ms_median=round(ms_old, 3), sdtw_ms_min=round(min_old, 3),
                            sdtw2_ms_median=round(ms_new, 3), sdtw2_ms_min=round(min_new, 3), ratio=round(ms_new / ms_old, 3),
                            sdtw_gcells_per_s=round(cells / ms_old / 1e6, 1), sdtw2_gcells_per_s=round(cells / ms_new / 1e6, 1),
                            rows_equal=bool(torch.equal(old, new)), reads_with_a_runner_up=int((sec[:, 1] >= 0).sum().item()),
                            mean_mapq=round(float(sec[:, 2].to(torch.float64).mean().item()), 2)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
