#!/usr/bin/env python3
"""What a round of the whole-read refine costs beside the band call it repeats and beside the table call whose passes it shares
(docs/codecs.md §4.24: k_path_fit_long, k_fit_long_solve, k_requant_long, k_refine_long_round).

  extend_refine_time.py [--reads 4096] [--events 16384] [--ref 65536] [--tile 256] [--band 512] [--reps 5] [--out FILE]

The input is that of tools/extend_time.py: reads that walk a reference of uniform int16 levels, made on the device with a fixed seed.  Then,
in ONE process, with the library's event hooks (hipEvent pairs on the null stream; median of --reps after 2 warm-ups):
  s5gpu_sdtw_band_dev              both passes: what a round repeats
  s5gpu_pileup_accum_long_dev      the whole call (no events) on the paths the band call left: the yardstick of a round's overhead, which
                                   reads the same arrays and runs the same plan and check passes
  s5gpu_extend_refine_dev          at iters 1 and 2
  ... its passes apart             refine_long_passes 1 (plan and check: round 0's and round 1's), 2 (k_path_fit_long and the clearing of the
                                   sums), 4 (k_fit_long_solve), 8 (k_requant_long), 16 (the bookkeeping: the fills, k_refine_long_gate,
                                   k_refine_long_round for rounds 0 and 1), 32 (the band call), at iters 1, over what a whole call left
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

EXT_ROW = np.dtype([("cost", "<u8"), ("qlen", "<u4"), ("tiles", "<u4"), ("start", "<i4"), ("end", "<i4"), ("a_last", "<i4"), ("status", "<i4")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--events", type=int, default=16384)
    ap.add_argument("--ref", type=int, default=65536)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--band", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    n, E, R, T, band = a.reads, a.events, a.ref, a.tile, a.band
    assert E % T == 0 and R > E + band
    total = n * E
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5105)
    ref = torch.randint(-127, 128, (R,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16).contiguous()
    s = torch.randint(band, R - E - band, (n,), generator=g, device="cuda", dtype=torch.int64)
    cols = s[:, None] + torch.cumsum(torch.randint(0, 2, (n, E), generator=g, device="cuda", dtype=torch.int8).to(torch.int32), 1)
    noise = torch.randint(-2, 3, (n, E), generator=g, device="cuda", dtype=torch.int32)
    q = (ref[cols].to(torch.int32) + noise).clamp_(-127, 127).to(torch.int16).contiguous().view(-1)
    del cols, noise
    first = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * E).contiguous()
    ql = torch.full((n,), E, dtype=torch.int32, device="cuda")
    anchor = s.to(torch.int32).contiguous()
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    bp = _lib.BandParams(0, 1, 1 << 20, T, band, 127, 32.0)
    sb = int(L.s5gpu_sdtw_band_scratch_bytes(n, total, T, band))
    scratch = torch.empty(sb // 4 + 4, dtype=torch.int32, device="cuda")
    rows = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    lo, hi = torch.zeros(total, dtype=torch.int32, device="cuda"), torch.zeros(total, dtype=torch.int32, device="cuda")
    res = []

    def opt(key, v):
        _lib.check(L.s5gpu_set_option(key, v), key.decode())

    def band_call():
        _lib.check(L.s5gpu_sdtw_band_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, anchor.data_ptr(), zero.data_ptr(), C.byref(bp),
                                         scratch.data_ptr(), sb, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(), None), "s5gpu_sdtw_band_dev")

    band_ms, band_min = timed(L, band_call, a.reps)
    torch.cuda.synchronize()
    h = rows.cpu().numpy().view(EXT_ROW).reshape(-1)
    common = dict(reads=n, events=E, R=R, tile=T, band=band)
    res.append(dict(kernel="s5gpu_sdtw_band_dev, both passes", ms_median=round(band_ms, 3), ms_min=round(band_min, 3), status_0=int((h["status"] == 0).sum()),
                    cost_per_event_mean=round(float((h["cost"] / np.maximum(h["qlen"], 1)).mean()), 3), **common))

    # the table call on the same paths
    need = int(L.s5gpu_pileup_long_work_bytes(n, total))
    pwork = torch.empty(need, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(int(L.s5gpu_pileup_bytes(R)), dtype=torch.uint8, device="cuda")
    _lib.check(L.s5gpu_pileup_reset_dev(acc.data_ptr(), R, None), "reset")

    def table_call():
        _lib.check(L.s5gpu_pileup_accum_long_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, lo.data_ptr(), hi.data_ptr(), zero.data_ptr(),
                                                 None, 0, pwork.data_ptr(), need, acc.data_ptr(), None), "s5gpu_pileup_accum_long_dev")

    table_ms, table_min = timed(L, table_call, a.reps)
    res.append(dict(kernel="s5gpu_pileup_accum_long_dev, the whole call, no events", ms_median=round(table_ms, 3), ms_min=round(table_min, 3)))
    del pwork, acc

    # the rounds
    wb = int(L.s5gpu_extend_refine_work_bytes(n, total))
    work = torch.empty(wb // 8 + 2, dtype=torch.int64, device="cuda")
    q1 = torch.zeros(total, dtype=torch.int16, device="cuda")
    rows1 = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    lo1, hi1 = torch.zeros(total, dtype=torch.int32, device="cuda"), torch.zeros(total, dtype=torch.int32, device="cuda")
    fit = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
    rounds = torch.zeros(n, dtype=torch.int32, device="cuda")

    def refine_call(iters):
        rp = _lib.RefineParams(0.5, 2.0, 64.0, 127, 16, 16, iters)

        def call():
            _lib.check(L.s5gpu_extend_refine_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                 C.byref(bp), C.byref(rp), scratch.data_ptr(), sb, work.data_ptr(), wb, q1.data_ptr(), rows1.data_ptr(), lo1.data_ptr(),
                                                 hi1.data_ptr(), fit.data_ptr(), rounds.data_ptr(), None), "s5gpu_extend_refine_dev")
        return call

    whole = {}
    for iters in (1, 2):
        whole[iters] = timed(L, refine_call(iters), a.reps)
        torch.cuda.synchronize()
        h1 = rows1.cpu().numpy().view(EXT_ROW).reshape(-1)
        f = fit.cpu().numpy().view(np.float64)
        res.append(dict(kernel="s5gpu_extend_refine_dev, iters %d" % iters, ms_median=round(whole[iters][0], 3), ms_min=round(whole[iters][1], 3),
                        status_0=int((h1["status"] == 0).sum()), rounds_mean=round(float(rounds.float().mean().item()), 3),
                        a_mean=round(float(f[:, 0].mean()), 4), b_mean=round(float(f[:, 1].mean()), 4),
                        cost_per_event_mean=round(float((h1["cost"] / np.maximum(h1["qlen"], 1)).mean()), 3), work_bytes=wb))
    parts = {}
    call = refine_call(1)
    for key, bits in (("plan_and_check_twice_ms", 1), ("k_path_fit_long_ms", 2), ("k_fit_long_solve_ms", 4), ("k_requant_long_ms", 8), ("bookkeeping_ms", 16),
                      ("band_call_ms", 32)):
        opt(b"refine_long_passes", 63)
        call()                                                             # (what the pass timed next works on)
        opt(b"refine_long_passes", bits)
        parts[key] = round(timed(L, call, a.reps)[0], 3)
    opt(b"refine_long_passes", 63)
    overhead = whole[1][0] - parts["band_call_ms"]
    res.append(dict(kernel="the passes of s5gpu_extend_refine_dev at iters 1, apart", **parts,
                    overhead_ms=round(overhead, 3), overhead_over_the_table_call=round(overhead / table_ms, 3),
                    a_round_over_the_band_call=round((whole[2][0] - whole[1][0]) / band_ms, 3), iters_1_over_the_band_call=round(whole[1][0] / band_ms, 3)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
