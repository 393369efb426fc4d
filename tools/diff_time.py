#!/usr/bin/env python3
"""What k_sig_diff costs beside a plain read of the same two slabs and beside k_file_stats (docs/codecs.md §4.14).

  diff_time.py [--reads 1000000] [--samples 4000] [--bits 3] [--reps 7] [--out FILE]

Synthetic reads (k_synth) are encoded on the device (zlib + svb-zd) and decoded once with S5GPU_DEC_NO_PAYLOAD: side A.  Side B is a second slab:
a copy of A rounded by s5gpu_qts_round_dev at --bits bits.  Then, in ONE run and one process, timed with the library's event hooks
(s5gpu_event_*; median of --reps launches after 2 warm-ups):
  read floor : k_read_floor over both slabs, every 16 bytes loaded once (s5tool_read_floor_dev, the hook of tools/fstats_time.py)
  fstats     : k_file_stats over side A alone (the figure of tools/fstats_time.py, measured again)
  diff       : k_sig_diff over the identity pairs with its defaults (rows and accumulator), without the accumulator (rows only: no
               histogram), and with no LDS bins (every differing sample a global 64-bit atomic) on a hundredth of the pairs
Bytes are the algorithm's: 2 N per read and side, once.  The accumulator of a default run over the first 100 000 pairs is checked against
torch.bincount and torch's sums of b - a, made on the device.  One JSON object per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, diff, fstats, press  # noqa: E402
from devtime import timed  # noqa: E402

HBM_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--bits", type=int, default=3)
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
    sig_a = torch.zeros(n_reads * sig_cap + 64, dtype=torch.int16, device="cuda")
    fields = torch.zeros(n_reads * 64, dtype=torch.uint8, device="cuda")
    L.s5gpu_decode_scratch_bytes.restype = C.c_uint64
    L.s5gpu_decode_scratch_bytes.argtypes = [C.c_uint32]
    sb = int(L.s5gpu_decode_scratch_bytes(pay_cap))
    scr = torch.empty(sb, dtype=torch.uint8, device="cuda")
    da = _lib.DecodeArgs()
    da.n_recs, da.rec_method, da.sig_method, da.flags = n_reads, 1, 1, _lib.DEC_NO_PAYLOAD
    da.desc, da.in_, da.sig_out, da.fields = desc.data_ptr(), b.stream_out.data_ptr(), sig_a.data_ptr(), fields.data_ptr()
    da.payload, da.payload_bytes, da.max_pay_cap, da.max_in_len = scr.data_ptr(), sb, pay_cap, int(d["in_len"].max())
    _lib.check(L.s5gpu_decode_dev(C.byref(da), None), "s5gpu_decode_dev")
    torch.cuda.synchronize()
    assert bool((fields.view(torch.int32).view(n_reads, 16)[:, 0] == 0).all().item())
    t_off = torch.from_numpy(d["sig_off"].astype(np.uint64).view(np.int64).copy()).cuda()
    t_cap = torch.from_numpy(d["sig_cap"].astype(np.uint32).view(np.int32).copy()).cuda()
    t_n = torch.full((n_reads,), n, dtype=torch.int32, device="cuda")
    sig_b = sig_a.clone()
    _lib.check(L.s5gpu_qts_round_dev(sig_b.data_ptr(), n_reads, t_off.data_ptr(), t_n.data_ptr(), a.bits, None), "s5gpu_qts_round_dev")
    torch.cuda.synchronize()
    del b, scr
    pairs = torch.arange(n_reads, dtype=torch.int32, device="cuda")
    rows = torch.zeros(n_reads * _lib.SIG_DIFF.itemsize, dtype=torch.uint8, device="cuda")
    fold = torch.zeros(4, dtype=torch.int32, device="cuda")
    facc, dacc = fstats.new_acc(), diff.new_acc()
    A, B = _lib.DiffSide(), _lib.DiffSide()
    for S, sig in ((A, sig_a), (B, sig_b)):
        S.n, S.sig, S.sig_off, S.sig_cap, S.fields = n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr()
    slab = 2 * n_reads * sig_cap
    nbytes = 2 * 2 * n * n_reads

    def floor():
        _lib.check(L.s5tool_read_floor_dev(sig_a.data_ptr(), slab, fold.data_ptr(), None), "s5tool_read_floor_dev")
        _lib.check(L.s5tool_read_floor_dev(sig_b.data_ptr(), slab, fold.data_ptr(), None), "s5tool_read_floor_dev")

    def accum():
        _lib.check(L.s5gpu_file_stats_accum_dev(n_reads, sig_a.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), facc.data_ptr(), None),
                   "s5gpu_file_stats_accum_dev")

    def sig_diff(m=n_reads, acc=dacc):
        _lib.check(L.s5gpu_signal_diff_dev(m, pairs.data_ptr(), pairs.data_ptr(), C.byref(A), C.byref(B), rows.data_ptr(),
                                           acc.data_ptr() if acc is not None else None, None), "s5gpu_signal_diff_dev")

    res = []
    fl_ms, fl_min = timed(L, floor, a.reps)
    res.append(dict(kernel="k_read_floor (16-byte loads), both slabs", bytes=2 * slab, ms_median=round(fl_ms, 3), ms_min=round(fl_min, 3),
                    tb_per_s=round(2 * slab / fl_ms / 1e9, 3), frac_of_6_29=round(2 * slab / fl_ms / 1e9 / HBM_TBS, 3)))
    fs_ms, fs_min = timed(L, accum, a.reps)
    res.append(dict(kernel="k_file_stats (defaults), side A alone", reads=n_reads, samples=n, bytes=nbytes // 2, ms_median=round(fs_ms, 3), ms_min=round(fs_min, 3),
                    tb_per_s=round(nbytes / 2 / fs_ms / 1e9, 3)))
    df_ms, df_min = timed(L, sig_diff, a.reps)
    # the check: the first pairs into a fresh accumulator against torch.bincount and torch's sums of b - a, on the device
    m = min(n_reads, 100_000)
    _lib.check(L.s5gpu_diff_acc_reset_dev(dacc.data_ptr(), None), "s5gpu_diff_acc_reset_dev")
    sig_diff(m)
    torch.cuda.synchronize()
    got = diff.to_numpy(dacc)
    xa = sig_a[: m * sig_cap].view(m, sig_cap)[:, :n].to(torch.int64)
    dd = sig_b[: m * sig_cap].view(m, sig_cap)[:, :n].to(torch.int64) - xa
    hist = torch.bincount((dd.reshape(-1) + 65535), minlength=131071).cpu().numpy()
    ok = bool(np.array_equal(got["hist"], hist.astype(np.uint64))) and int(got["n_pairs"]) == m and int(got["n_samples"]) == n * m
    ok &= int(got["sum_d"]) == int(dd.sum().item()) and int(got["sum_sq"]) == int((dd * dd).sum().item()) and int(got["sum_abs"]) == int(dd.abs().sum().item())
    ok &= int(got["n_diff"]) == int((dd != 0).sum().item()) and int(got["max_abs"]) == int(dd.abs().max().item())
    ok &= int(got["sum_a"]) == int(xa.sum().item()) and int(got["sumsq_a"]) == int((xa * xa).sum().item())
    r0 = rows[: m * 80].cpu().numpy().view(_lib.SIG_DIFF)
    ok &= int(r0["n_diff"].astype(np.int64).sum()) == int(got["n_diff"]) and bool((r0["flags"] <= 1).all())
    levels = int((hist > 0).sum())
    res.append(dict(kernel="k_sig_diff (defaults: rows + accumulator)", pairs=n_reads, samples=n, bits=a.bits, ms_median=round(df_ms, 3), ms_min=round(df_min, 3),
                    bytes=nbytes, tb_per_s=round(nbytes / df_ms / 1e9, 3), frac_of_6_29=round(nbytes / df_ms / 1e9 / HBM_TBS, 3),
                    over_floor=round(df_ms / fl_ms, 2), over_k_file_stats=round(df_ms / fs_ms, 2), differences_in_use=levels,
                    frac_samples_differ=round(int(got["n_diff"]) / (n * m), 4), max_abs=int(got["max_abs"]), matches_device_bincount=bool(ok)))
    nr_ms, nr_min = timed(L, lambda: sig_diff(n_reads, None), a.reps)
    res.append(dict(kernel="k_sig_diff (rows only: no accumulator, no histogram)", pairs=n_reads, samples=n, ms_median=round(nr_ms, 3), ms_min=round(nr_min, 3),
                    over_floor=round(nr_ms / fl_ms, 2)))
    part = max(n_reads // 100, 1)
    _lib.check(L.s5gpu_set_option(b"diff_lds_bins", 0))
    g_ms, g_min = timed(L, lambda: sig_diff(part), max(a.reps // 2, 1), warm=1)
    _lib.check(L.s5gpu_set_option(b"diff_lds_bins", 64))
    res.append(dict(kernel="k_sig_diff (no LDS bins: global atomics only)", pairs=part, samples=n, ms_median=round(g_ms, 3), ms_min=round(g_min, 3),
                    ms_per_pair_over_default=round((g_ms / part) / (df_ms / n_reads), 1)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
