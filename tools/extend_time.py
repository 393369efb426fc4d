#!/usr/bin/env python3
"""What the banded alignment of whole reads costs beside the window call on the same number of cells, and beside the mapping that anchors
it (docs/codecs.md §4.21: k_sdtw_band, k_sdtw_band_trace).

  extend_time.py [--reads 4096] [--events 16384] [--ref 65536] [--tile 256] [--band 512] [--reps 5] [--out FILE]

Synthetic reads are made on the device: a reference of uniform int16 levels in +-127 (a fixed seed), and per read a walk along it from a
random column that advances by 0 or 1 column an event, the level plus noise of +-2 as the event's value, so that the band tracks; the
anchor is the walk's first column.  Then, in ONE process, with the library's event hooks (hipEvent pairs on the null stream; median of
--reps after 2 warm-ups):
  s5gpu_sdtw_band_dev, pass 1        k_sdtw_band alone (option sdtw_band_passes = 1): cells = sum of rows x W_k
  s5gpu_sdtw_band_dev, pass 2        k_sdtw_band_trace alone, over what pass 1 left
  s5gpu_sdtw_band_dev                both
  s5gpu_sdtw_window_dev              the yardstick: the same values as queries of `tile` rows, each against a window of `band` columns
                                     placed where the walk is (pad 0), so the same number of cells; its trace is part of the call
  s5gpu_sdtw_dev, 250 rows           the mapping of a 250-event prefix of every read against the whole reference, with the start
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
    tile_col = cols[:, ::T].contiguous().view(-1)                            # the walk's column at the first row of every tile
    last_col = cols[:, -1].cpu().numpy()
    del cols, noise
    first = (torch.arange(n + 1, device="cuda", dtype=torch.int64) * E).contiguous()
    ql = torch.full((n,), E, dtype=torch.int32, device="cuda")
    anchor = s.to(torch.int32).contiguous()
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    p = _lib.BandParams(0, 1, 1 << 20, T, band, 127, 32.0)
    sb = int(L.s5gpu_sdtw_band_scratch_bytes(n, total, T, band))
    scratch = torch.empty(sb // 4 + 4, dtype=torch.int32, device="cuda")
    rows = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    lo, hi = torch.zeros(total, dtype=torch.int32, device="cuda"), torch.zeros(total, dtype=torch.int32, device="cuda")
    res = []

    def band_call():
        _lib.check(L.s5gpu_sdtw_band_dev(n, q.data_ptr(), first.data_ptr(), ql.data_ptr(), total, ref.data_ptr(), R, anchor.data_ptr(), zero.data_ptr(), C.byref(p),
                                         scratch.data_ptr(), sb, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(), None), "s5gpu_sdtw_band_dev")

    out = {}
    for name, passes in (("k_sdtw_band", 1), ("k_sdtw_band_trace", 2), ("both", 3)):
        _lib.check(L.s5gpu_set_option(b"sdtw_band_passes", passes), "s5gpu_set_option")
        if passes == 2:
            _lib.check(L.s5gpu_set_option(b"sdtw_band_passes", 1)); band_call(); _lib.check(L.s5gpu_set_option(b"sdtw_band_passes", 2))
        out[name] = timed(L, band_call, a.reps)
    _lib.check(L.s5gpu_set_option(b"sdtw_band_passes", 3))
    torch.cuda.synchronize()
    h = rows.cpu().numpy().view(np.dtype([("cost", "<u8"), ("qlen", "<u4"), ("tiles", "<u4"), ("start", "<i4"), ("end", "<i4"), ("a_last", "<i4"), ("status", "<i4")])).reshape(-1)
    cells = total * band                                                   # (every window is `band` wide: the walks keep clear of the reference's ends)
    tracked = float((np.abs(h["end"].astype(np.int64) - last_col) <= 2).mean())
    res.append(dict(kernel="s5gpu_sdtw_band_dev pass 1 (k_sdtw_band<%d>)" % (T // 64), reads=n, events=E, R=R, tile=T, band=band, band_cells=cells, scratch_bytes=sb,
                    ms_median=round(out["k_sdtw_band"][0], 3), ms_min=round(out["k_sdtw_band"][1], 3),
                    gcells_per_s=round(cells / out["k_sdtw_band"][0] / 1e6, 1)))
    res.append(dict(kernel="s5gpu_sdtw_band_dev pass 2 (k_sdtw_band_trace)", ms_median=round(out["k_sdtw_band_trace"][0], 3), ms_min=round(out["k_sdtw_band_trace"][1], 3)))
    res.append(dict(kernel="s5gpu_sdtw_band_dev, both passes", ms_median=round(out["both"][0], 3), ms_min=round(out["both"][1], 3), status_0=int((h["status"] == 0).sum()),
                    cost_per_event_mean=round(float((h["cost"] / np.maximum(h["qlen"], 1)).mean()), 3), tiles=int(h["tiles"].sum()),
                    end_within_2_of_the_walk=tracked))
    # the yardstick: the window call on the same values and the same number of cells
    nt = n * (E // T)
    qt = q.view(nt, T)
    qlt = torch.full((nt,), T, dtype=torch.int32, device="cuda")
    ws = (tile_col - band // 4).clamp_(0, R - band).to(torch.int32)
    rin = torch.stack([torch.zeros_like(ws), torch.full_like(ws, T), ws, ws + (band - 1)], 1).contiguous()
    rout = torch.zeros((nt, 4), dtype=torch.int32, device="cuda")
    lo2, hi2, st2 = torch.zeros((nt, T), dtype=torch.int32, device="cuda"), torch.zeros((nt, T), dtype=torch.int32, device="cuda"), torch.zeros(nt, dtype=torch.int32, device="cuda")
    slot = int(L.s5gpu_sdtw_path_slot_bytes(T, band))
    wsb = min(slot * nt, scratch.numel() * 4 - 16)

    def window_call():
        _lib.check(L.s5gpu_sdtw_window_dev(nt, qt.data_ptr(), T, qlt.data_ptr(), ref.data_ptr(), R, rin.data_ptr(), 0, band, scratch.data_ptr(), wsb, rout.data_ptr(),
                                           lo2.data_ptr(), hi2.data_ptr(), st2.data_ptr(), None), "s5gpu_sdtw_window_dev")
    w_ms, w_min = timed(L, window_call, a.reps)
    torch.cuda.synchronize()
    res.append(dict(kernel="s5gpu_sdtw_window_dev (k_sdtw_win<%d>, k_sdtw_trace_win), pad 0" % (T // 64), queries=nt, rows=T, window=band, cells=nt * T * band,
                    groups=-(-slot * nt // wsb), ms_median=round(w_ms, 3), ms_min=round(w_min, 3), gcells_per_s=round(nt * T * band / w_ms / 1e6, 1),
                    status_0=int((st2 == 0).sum().item()), band_call_over_window_call=round(out["both"][0] / w_ms, 3),
                    band_pass_1_over_window_call=round(out["k_sdtw_band"][0] / w_ms, 3)))
    # the mapping that anchors a read: 250 rows against the whole reference
    Qm = 250
    qm = q.view(n, E)[:, :Qm].contiguous()
    qlm = torch.full((n,), Qm, dtype=torch.int32, device="cuda")
    mrows = torch.zeros((n, 4), dtype=torch.int32, device="cuda")

    def map_call():
        _lib.check(L.s5gpu_sdtw_dev(n, qm.data_ptr(), Qm, qlm.data_ptr(), ref.data_ptr(), R, 1, mrows.data_ptr(), None), "s5gpu_sdtw_dev")
    m_ms, m_min = timed(L, map_call, a.reps)
    torch.cuda.synchronize()
    found = float((mrows[:, 2].to(torch.int64) - s).abs().le(2).float().mean().item())
    per_read_band = out["both"][0] / n * (20000.0 / E)
    res.append(dict(kernel="s5gpu_sdtw_dev (k_sdtw, want_start), 250 rows", reads=n, cells=n * Qm * R, ms_median=round(m_ms, 3), ms_min=round(m_min, 3),
                    gcells_per_s=round(n * Qm * R / m_ms / 1e6, 1), start_within_2_of_the_walk=found,
                    a_20000_event_read_band_us=round(per_read_band * 1e3, 3), its_250_event_mapping_us=round(m_ms / n * 1e3, 3),
                    band_over_mapping=round(per_read_band / (m_ms / n), 3)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
