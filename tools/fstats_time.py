#!/usr/bin/env python3
"""What the file-wide accumulator costs beside k_sig_stats and a plain read of the same samples (docs/codecs.md §4.13, k_file_stats).

  fstats_time.py [--reads 1000000] [--samples 4000] [--reps 7] [--out FILE]

Synthetic reads (k_synth) are encoded on the device (zlib + svb-zd) and decoded once with S5GPU_DEC_NO_PAYLOAD; then, in ONE run and on the
same decoded signals, timed with the library's event hooks (s5gpu_event_*; median of --reps launches after 2 warm-ups):
  read floor : k_read_floor, every 16 bytes of the signal slots loaded once (s5tool_read_floor_dev, a hook of this tool in fstats_kernels.hip)
  stats      : k_sig_stats, quantiles (0.2, 0.9) (the figure of tools/signals_time.py, measured again)
  fstats     : k_file_stats with its defaults, and with no LDS bins (every sample a global 64-bit atomic) on a hundredth of the reads
Bytes are the algorithm's: 2 N per read, once.  The accumulator of a default run is checked against torch.bincount and torch's sums
of every decoded sample, made on the device.  One JSON object per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, fstats, press, signals  # noqa: E402
from devtime import timed  # noqa: E402

HBM_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
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
    t_off = torch.from_numpy(d["sig_off"].astype(np.uint64).view(np.int64).copy()).cuda()
    t_cap = torch.from_numpy(d["sig_cap"].astype(np.uint32).view(np.int32).copy()).cuda()
    t_stats = torch.zeros(n_reads * signals.SIG_STATS.itemsize, dtype=torch.uint8, device="cuda")
    q = (C.c_double * 2)(0.2, 0.9)
    fold = torch.zeros(4, dtype=torch.int32, device="cuda")
    acc = fstats.new_acc()
    nbytes = 2 * n * n_reads

    def floor():
        _lib.check(L.s5tool_read_floor_dev(sig.data_ptr(), 2 * n_reads * sig_cap, fold.data_ptr(), None), "s5tool_read_floor_dev")

    def stats():
        _lib.check(L.s5gpu_signal_stats_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), 2, q, t_stats.data_ptr(), None),
                   "s5gpu_signal_stats_dev")

    def accum(m=n_reads):
        _lib.check(L.s5gpu_file_stats_accum_dev(m, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), acc.data_ptr(), None),
                   "s5gpu_file_stats_accum_dev")

    res = []
    fl_ms, fl_min = timed(L, floor, a.reps)
    res.append(dict(kernel="k_read_floor (16-byte loads)", bytes=2 * n_reads * sig_cap, ms_median=round(fl_ms, 3), ms_min=round(fl_min, 3),
                    tb_per_s=round(2 * n_reads * sig_cap / fl_ms / 1e9, 3), frac_of_6_29=round(2 * n_reads * sig_cap / fl_ms / 1e9 / HBM_TBS, 3)))
    st_ms, st_min = timed(L, stats, a.reps)
    res.append(dict(kernel="k_sig_stats", reads=n_reads, samples=n, ms_median=round(st_ms, 3), ms_min=round(st_min, 3), over_floor=round(st_ms / fl_ms, 2)))
    fs_ms, fs_min = timed(L, accum, a.reps)
    # the check: one accumulation into a fresh accumulator against torch.bincount and torch's sums of every sample, on the device
    _lib.check(L.s5gpu_file_stats_reset_dev(acc.data_ptr(), None), "s5gpu_file_stats_reset_dev")
    accum()
    torch.cuda.synchronize()
    got = fstats.to_numpy(acc)
    x = sig[: n_reads * sig_cap].view(n_reads, sig_cap)[:, :n]
    hist = torch.bincount((x.reshape(-1).to(torch.int32) + 32768), minlength=65536).cpu().numpy()
    x64 = x.to(torch.int64)
    ok = bool(np.array_equal(got["hist"], hist.astype(np.uint64))) and int(got["n_reads"]) == n_reads and int(got["n_samples"]) == n * n_reads
    ok &= int(got["sum"]) == int(x64.sum().item()) and int(got["sumsq"]) == int((x64 * x64).sum().item()) & (2 ** 64 - 1)
    ok &= int(got["min"]) == int(x.min().item()) and int(got["max"]) == int(x.max().item()) and int(got["len_hist"][int(n).bit_length()]) == n_reads
    levels = int((hist > 0).sum())
    res.append(dict(kernel="k_file_stats (defaults)", reads=n_reads, samples=n, ms_median=round(fs_ms, 3), ms_min=round(fs_min, 3), bytes=nbytes,
                    tb_per_s=round(nbytes / fs_ms / 1e9, 3), frac_of_6_29=round(nbytes / fs_ms / 1e9 / HBM_TBS, 3), over_floor=round(fs_ms / fl_ms, 2),
                    over_k_sig_stats=round(fs_ms / st_ms, 3), levels_in_use=levels, sample_min=int(got["min"]), sample_max=int(got["max"]),
                    matches_device_bincount=bool(ok)))
    part = max(n_reads // 100, 1)
    _lib.check(L.s5gpu_set_option(b"fstats_lds_bins", 0))
    g_ms, g_min = timed(L, lambda: accum(part), max(a.reps // 2, 1), warm=1)
    _lib.check(L.s5gpu_set_option(b"fstats_lds_bins", 2048))
    res.append(dict(kernel="k_file_stats (no LDS bins: global atomics only)", reads=part, samples=n, ms_median=round(g_ms, 3), ms_min=round(g_min, 3),
                    ms_per_read_over_default=round((g_ms / part) / (fs_ms / n_reads), 1)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
