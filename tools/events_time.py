#!/usr/bin/env python3
"""What event segmentation costs beside k_sig_stats and a plain read of the same samples (docs/codecs.md §4.15, k_sig_events).

  events_time.py [--reads 1000000] [--samples 4000] [--reps 5] [--rna] [--out FILE]

Synthetic reads (k_synth) are encoded on the device (zlib + svb-zd) and decoded once with S5GPU_DEC_NO_PAYLOAD; then, in ONE run and on the
same decoded signals, timed with the library's event hooks (s5gpu_event_*; median of --reps launches after 2 warm-ups):
  read floor : k_read_floor, every 16 bytes of the signal slots loaded once (s5tool_read_floor_dev)
  stats      : k_sig_stats, quantiles (0.2, 0.9)
  count      : k_sig_events with rows = NULL
  fill       : k_sig_events into slots sized by the count pass (raw mode)
  both       : count, torch.cumsum, fill — what events_dev runs, without the allocation of the rows
Bytes are the algorithm's: 2 N per read in, 16 per event out.  The counts of the two passes are compared, and the rows of the first reads
are checked for tiling [0, n).  One JSON object per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, events, press, signals  # noqa: E402
from devtime import timed  # noqa: E402

HBM_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rna", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
    L.s5tool_read_floor_dev.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    n_reads, n = a.reads, a.samples
    b = press.DeviceBatch(np.full(n_reads, n, dtype=np.uint64))
    b.synth(); b.encode_stream(); torch.cuda.synchronize()
    assert b.stream_ok()
    off = b.rec_off.cpu().numpy().astype(np.int64)
    pay_cap = 16 * ((int(b.tot["max_payload"]) + 31) // 16)
    sig_cap = (n + 7) // 8 * 8
    d = np.zeros(n_reads, dtype=_lib.REC_DESC)
    d["in_off"], d["in_len"] = off[:-1] + 8, np.diff(off) - 8
    d["sig_off"], d["sig_cap"] = np.arange(n_reads, dtype=np.uint64) * sig_cap, sig_cap
    desc = torch.from_numpy(d.view(np.uint8).copy()).cuda()
    sig = torch.zeros(n_reads * sig_cap + 64, dtype=torch.int16, device="cuda")
    fields = torch.zeros(n_reads * 64, dtype=torch.uint8, device="cuda")
    L.s5gpu_decode_scratch_bytes.restype = C.c_uint64
    L.s5gpu_decode_scratch_bytes.argtypes = [C.c_uint32]
    sb = int(L.s5gpu_decode_scratch_bytes(pay_cap))
    scr = torch.empty(sb, dtype=torch.uint8, device="cuda")
    da = _lib.DecodeArgs()
    da.n_recs, da.rec_method, da.sig_method, da.flags = n_reads, 1, 1, _lib.DEC_NO_PAYLOAD
    da.desc, da.in_, da.sig_out, da.fields = desc.data_ptr(), b.stream_out.data_ptr(), sig.data_ptr(), fields.data_ptr()
    da.payload, da.payload_bytes, da.max_pay_cap, da.max_in_len = scr.data_ptr(), sb, pay_cap, int(d["in_len"].max())
    _lib.check(L.s5gpu_decode_dev(C.byref(da), None), "s5gpu_decode_dev")
    torch.cuda.synchronize()
    assert bool((fields.view(torch.int32).view(n_reads, 16)[:, 0] == 0).all().item())
    del b, scr
    t_off = torch.from_numpy(d["sig_off"].astype(np.uint64).view(np.int64).copy()).cuda()
    t_cap = torch.from_numpy(d["sig_cap"].astype(np.uint32).view(np.int32).copy()).cuda()
    t_stats = torch.zeros(n_reads * signals.SIG_STATS.itemsize, dtype=torch.uint8, device="cuda")
    q = (C.c_double * 2)(0.2, 0.9)
    fold = torch.zeros(4, dtype=torch.int32, device="cuda")
    params = events.RNA if a.rna else events.DNA
    p = _lib.EventParams(*params)
    cnt = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    cnt2 = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    st = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    first = torch.zeros(n_reads + 1, dtype=torch.int64, device="cuda")
    nbytes = 2 * n * n_reads

    def floor():
        _lib.check(L.s5tool_read_floor_dev(sig.data_ptr(), 2 * n_reads * sig_cap, fold.data_ptr(), None), "s5tool_read_floor_dev")

    def stats():
        _lib.check(L.s5gpu_signal_stats_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), 2, q, t_stats.data_ptr(), None),
                   "s5gpu_signal_stats_dev")

    def count():
        _lib.check(L.s5gpu_signal_events_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), C.byref(p), 0,
                                             None, None, None, cnt.data_ptr(), st.data_ptr(), None), "s5gpu_signal_events_dev (count)")

    def scan():
        first[1:] = torch.cumsum(cnt.to(torch.int64), 0)

    res = []
    fl_ms, fl_min = timed(L, floor, a.reps)
    res.append(dict(kernel="k_read_floor (16-byte loads)", bytes=2 * n_reads * sig_cap, ms_median=round(fl_ms, 3), ms_min=round(fl_min, 3),
                    tb_per_s=round(2 * n_reads * sig_cap / fl_ms / 1e9, 3), frac_of_6_29=round(2 * n_reads * sig_cap / fl_ms / 1e9 / HBM_TBS, 3)))
    st_ms, st_min = timed(L, stats, a.reps)
    res.append(dict(kernel="k_sig_stats", reads=n_reads, samples=n, ms_median=round(st_ms, 3), ms_min=round(st_min, 3), over_floor=round(st_ms / fl_ms, 2)))
    c_ms, c_min = timed(L, count, a.reps)
    scan()
    total = int(first[n_reads].item())
    rows = torch.zeros((total, 4), dtype=torch.int32, device="cuda")

    def fill():
        _lib.check(L.s5gpu_signal_events_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), C.byref(p), 0,
                                             first.data_ptr(), cnt.data_ptr(), rows.data_ptr(), cnt2.data_ptr(), st.data_ptr(), None),
                   "s5gpu_signal_events_dev (fill)")

    def both():
        count(); scan(); fill()

    f_ms, f_min = timed(L, fill, a.reps)
    b_ms, b_min = timed(L, both, a.reps)
    torch.cuda.synchronize()
    same = bool(torch.equal(cnt, cnt2)) and not bool(st.any().item())
    k = min(n_reads, 64)
    fi = first[:k + 1].cpu().numpy()
    hr = rows[:int(fi[k])].cpu().numpy().view(np.uint32)
    tiles = all(hr[fi[i], 0] == 0 and (hr[fi[i]:fi[i + 1], 0][1:] == (hr[fi[i]:fi[i + 1], 0] + hr[fi[i]:fi[i + 1], 1])[:-1]).all()
                and hr[fi[i + 1] - 1, 0] + hr[fi[i + 1] - 1, 1] == n for i in range(k))
    common = dict(reads=n_reads, samples=n, params=list(params), events=total, events_per_read=round(total / n_reads, 1))
    res.append(dict(kernel="k_sig_events (count pass)", **common, ms_median=round(c_ms, 3), ms_min=round(c_min, 3), bytes=nbytes,
                    tb_per_s=round(nbytes / c_ms / 1e9, 3), gsamples_per_s=round(n * n_reads / c_ms / 1e6, 1), over_floor=round(c_ms / fl_ms, 2),
                    over_k_sig_stats=round(c_ms / st_ms, 2)))
    res.append(dict(kernel="k_sig_events (fill pass)", **common, ms_median=round(f_ms, 3), ms_min=round(f_min, 3), bytes=nbytes + 16 * total,
                    tb_per_s=round((nbytes + 16 * total) / f_ms / 1e9, 3), gsamples_per_s=round(n * n_reads / f_ms / 1e6, 1),
                    over_floor=round(f_ms / fl_ms, 2), over_k_sig_stats=round(f_ms / st_ms, 2), counts_match_the_count_pass=same, rows_tile_the_reads=bool(tiles)))
    res.append(dict(kernel="count + cumsum + fill", **common, ms_median=round(b_ms, 3), ms_min=round(b_min, 3), over_floor=round(b_ms / fl_ms, 2),
                    over_k_sig_stats=round(b_ms / st_ms, 2)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
