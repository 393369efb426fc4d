#!/usr/bin/env python3
"""What the path of an alignment costs beside the mapping that found it (docs/codecs.md §4.17, k_sdtw_dirs and k_sdtw_trace).

  sdtw_path_time.py [--reads 65536] [--qlen 256] [--ref 65536] [--wmax 0] [--scratch-mb 0] [--reps 5] [--out FILE]

Synthetic queries and a reference (uniform int16 in +-127, a fixed seed) are made on the device; then, in ONE process, with the library's
event hooks (s5gpu_event_*; median of --reps after 2 warm-ups):
  s5gpu_sdtw_dev with want_start   the yardstick, and where the rows come from: reads x qlen x ref cells
  s5gpu_sdtw_path_dev, dirs only   option sdtw_path_passes = 1: a launch per lane height the pitch allows, the recurrence over the window
  s5gpu_sdtw_path_dev, trace only  option sdtw_path_passes = 2: the walk over what the dirs pass left in the scratch
  s5gpu_sdtw_path_dev              both, the call as users make it
The dirs pass is rated in window cells (the sum of qlen x (end - start + 1) over the reads with a path) per second against the yardstick's
cells per second.  --wmax 0: 4 qlen.  --scratch-mb 0: a slot for every read (one group).
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
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--wmax", type=int, default=0)
    ap.add_argument("--scratch-mb", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, Q, R = a.reads, a.qlen, a.ref
    wmax = a.wmax or 4 * Q
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    q = torch.randint(-127, 128, (n, Q), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    ql = torch.full((n,), Q, dtype=torch.int32, device="cuda")
    ref = torch.randint(-127, 128, (R,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    rows = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    lo = torch.zeros((n, Q), dtype=torch.int32, device="cuda")
    hi = torch.zeros((n, Q), dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    slot = int(L.s5gpu_sdtw_path_slot_bytes(Q, wmax))
    sb = (a.scratch_mb << 20) if a.scratch_mb else slot * n
    scratch = torch.empty(sb // 4 + 4, dtype=torch.int32, device="cuda")
    lane_height = next(h for h in (1, 2, 4, 8, 16) if 64 * h >= Q)
    res = []

    def sdtw():
        _lib.check(L.s5gpu_sdtw_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, 1, rows.data_ptr(), None), "s5gpu_sdtw_dev")

    def path():
        _lib.check(L.s5gpu_sdtw_path_dev(n, q.data_ptr(), Q, ql.data_ptr(), ref.data_ptr(), R, rows.data_ptr(), wmax, scratch.data_ptr(), sb, lo.data_ptr(),
                                         hi.data_ptr(), st.data_ptr(), None), "s5gpu_sdtw_path_dev")

    ms, ms_min = timed(L, sdtw, a.reps)
    cells = n * Q * R
    yard = cells / ms / 1e6
    res.append(dict(kernel="k_sdtw<%d, true>" % lane_height, reads=n, qlen=Q, R=R, cells=cells, ms_median=round(ms, 3), ms_min=round(ms_min, 3),
                    gcells_per_s=round(yard, 1)))
    torch.cuda.synchronize()
    h = rows.cpu().numpy()
    span = (h[:, 3] - h[:, 2] + 1).astype(np.int64)
    has = span <= wmax
    wcells = int((span[has] * Q).sum())
    common = dict(reads=n, qlen=Q, wmax=wmax, slot_bytes=slot, scratch_bytes=sb, groups=-(-n // max(1, min(n, sb // slot))), reads_with_a_path=int(has.sum()),
                  span_mean=round(float(span.mean()), 1), span_max=int(span.max()), window_cells=wcells)
    for passes, name in ((1, "k_sdtw_dirs<%d>" % lane_height), (2, "k_sdtw_trace"), (3, "s5gpu_sdtw_path_dev")):
        _lib.check(L.s5gpu_set_option(b"sdtw_path_passes", 3), "opt")
        path()                                                            # (the scratch and the outputs as a whole call leaves them)
        _lib.check(L.s5gpu_set_option(b"sdtw_path_passes", passes), "opt")
        ms, ms_min = timed(L, path, a.reps)
        r = dict(kernel=name, ms_median=round(ms, 3), ms_min=round(ms_min, 3), **common)
        if passes == 1:
            r["window_gcells_per_s"] = round(wcells / ms / 1e6, 1)
            r["cells_per_s_against_k_sdtw_true"] = round(wcells / ms / 1e6 / yard, 3)
        if passes == 3:
            r["path_call_over_mapping"] = round(ms / res[0]["ms_median"], 4)
        res.append(r)
    _lib.check(L.s5gpu_set_option(b"sdtw_path_passes", 3), "opt")
    torch.cuda.synchronize()
    h_st, h_lo, h_hi = st.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy()
    ok = h_st == 0
    res[-1]["status_counts"] = {str(int(k)): int(v) for k, v in zip(*np.unique(h_st, return_counts=True))}
    res[-1]["ends_agree_with_rows"] = bool(np.array_equal(ok, has) and (h_lo[ok, 0] == h[ok, 2]).all() and (h_hi[ok, Q - 1] == h[ok, 3]).all()
                                           and (h_lo[~ok] == -1).all() and (h_hi[~ok] == -1).all())
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
