#!/usr/bin/env python3
"""What the signal kernels cost beside the decode that feeds them (k_sig_stats / k_sig_windows).

  signals_time.py [--reads 1000000] [--samples 4000] [--reps 7] [--out FILE]

Synthetic reads (k_synth) are encoded on the device (zlib + svb-zd), then, in ONE run and on the same reads, timed with the library's event
hooks (s5gpu_event_*; median of --reps launches after 2 warm-ups):
  decode   : s5gpu_decode_dev, S5GPU_DEC_NO_PAYLOAD (fields + signals into HBM)
  stats    : k_sig_stats, quantiles (0.2, 0.9)
  windows  : k_sig_windows, MEDMAD, float16, W = samples, one window per read (the padded batch)
Bytes are the algorithm's: stats reads 2N per pass, five passes (the re-reads of an 8 KB read come from L2: the compulsory HBM traffic is one
pass); windows reads 2N and writes 2 W per window (float16).  Shares are of 6.29 TB/s, the measured HBM copy rate.  The decoded signals are
checked against the generator and a few reads' statistics against numpy.  One JSON object per line; --out also writes them to a file."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slow5tools_amd import _lib, press, signals  # noqa: E402
from devtime import timed  # noqa: E402

HBM_TBS = 6.29
STATS_PASSES = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.check(L.s5gpu_init(0), "s5gpu_init")
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
    sig = torch.empty(n_reads * sig_cap + 64, dtype=torch.int16, device="cuda")
    fields = torch.zeros(n_reads * 64, dtype=torch.uint8, device="cuda")
    L.s5gpu_decode_scratch_bytes.restype = C.c_uint64
    L.s5gpu_decode_scratch_bytes.argtypes = [C.c_uint32]
    sb = int(L.s5gpu_decode_scratch_bytes(pay_cap))
    scr = torch.empty(sb, dtype=torch.uint8, device="cuda")
    da = _lib.DecodeArgs()
    da.n_recs, da.rec_method, da.sig_method, da.flags = n_reads, 1, 1, _lib.DEC_NO_PAYLOAD
    da.desc, da.in_, da.sig_out, da.fields = desc.data_ptr(), b.stream_out.data_ptr(), sig.data_ptr(), fields.data_ptr()
    da.payload, da.payload_bytes, da.max_pay_cap, da.max_in_len = scr.data_ptr(), sb, pay_cap, int(d["in_len"].max())
    t_off = torch.from_numpy(d["sig_off"].astype(np.uint64).view(np.int64).copy()).cuda()
    t_cap = torch.from_numpy(d["sig_cap"].astype(np.uint32).view(np.int32).copy()).cuda()
    t_stats = torch.zeros(n_reads * signals.SIG_STATS.itemsize, dtype=torch.uint8, device="cuda")
    q = (C.c_double * 2)(0.2, 0.9)
    W = n
    out = torch.empty((n_reads, W), dtype=torch.float16, device="cuda")
    wr = torch.arange(n_reads, dtype=torch.int32, device="cuda")
    ws = torch.zeros(n_reads, dtype=torch.int32, device="cuda")
    wst = torch.zeros(n_reads, dtype=torch.int32, device="cuda")

    def decode():
        _lib.check(L.s5gpu_decode_dev(C.byref(da), None), "s5gpu_decode_dev")

    def stats():
        _lib.check(L.s5gpu_signal_stats_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), 2, q, t_stats.data_ptr(), None),
                   "s5gpu_signal_stats_dev")

    def windows():
        _lib.check(L.s5gpu_signal_windows_dev(n_reads, sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), fields.data_ptr(), t_stats.data_ptr(), n_reads,
                                              wr.data_ptr(), ws.data_ptr(), W, _lib.NORM_MEDMAD, 0.0, 0.0, _lib.SIG_F16, out.data_ptr(), wst.data_ptr(), None),
                   "s5gpu_signal_windows_dev")

    res = []
    dec_ms, dec_min = timed(L, decode, a.reps)
    st = fields.view(torch.int32).view(n_reads, 16)[:, 0]
    same = bool((st == 0).all().item()) and bool(torch.equal(sig[: n_reads * sig_cap].view(n_reads, sig_cap)[:, :n], b.sig[: n_reads * sig_cap].view(n_reads, sig_cap)[:, :n]))
    z = int(off[-1])
    res.append(dict(kernel="decode (S5GPU_DEC_NO_PAYLOAD)", reads=n_reads, samples=n, ms_median=round(dec_ms, 3), ms_min=round(dec_min, 3),
                    reads_per_s=round(n_reads / dec_ms * 1e3), bytes=z + 2 * n * n_reads, signals_identical=same))
    st_ms, st_min = timed(L, stats, a.reps)
    hs = t_stats[: 8 * signals.SIG_STATS.itemsize].cpu().numpy().view(signals.SIG_STATS)
    hx = sig[: 8 * sig_cap].cpu().numpy().reshape(8, sig_cap)[:, :n].astype(np.int64)
    ok = True
    for i in range(min(8, n_reads)):
        s = np.sort(hx[i]); med2 = int(s[(n - 1) // 2] + s[n // 2]); ks = np.sort(np.abs(2 * hx[i] - med2))
        ok &= int(hs["med2"][i]) == med2 and int(hs["mad4"][i]) == int(ks[(n - 1) // 2] + ks[n // 2]) and int(hs["sum"][i]) == int(hx[i].sum())
        ok &= int(hs["q"][i][0]) == int(s[int(np.floor(0.2 * (n - 1)))]) and int(hs["q"][i][1]) == int(s[int(np.floor(0.9 * (n - 1)))])
    sbytes = STATS_PASSES * 2 * n * n_reads
    res.append(dict(kernel="k_sig_stats", reads=n_reads, samples=n, ms_median=round(st_ms, 3), ms_min=round(st_min, 3), passes=STATS_PASSES,
                    algorithmic_bytes=sbytes, algorithmic_tb_per_s=round(sbytes / st_ms / 1e9, 3), compulsory_bytes=2 * n * n_reads,
                    compulsory_frac_of_6_29=round(2 * n * n_reads / st_ms / 1e9 / HBM_TBS, 3), of_decode=round(st_ms / dec_ms, 3), first_reads_match_numpy=bool(ok)))
    w_ms, w_min = timed(L, windows, a.reps)
    wbytes = 2 * n * n_reads + 2 * W * n_reads
    row = out[0].float().cpu().numpy()
    want = (2.0 * hx[0] - int(hs["med2"][0])) / (0.7413 * int(hs["mad4"][0]) if int(hs["mad4"][0]) else 1.0)
    wok = bool(np.allclose(row, want.astype(np.float32).astype(np.float16).astype(np.float32), rtol=2e-3, atol=0)) and int(wst.sum().item()) == 0
    res.append(dict(kernel="k_sig_windows (MEDMAD, float16, W=%d)" % W, windows=n_reads, ms_median=round(w_ms, 3), ms_min=round(w_min, 3), bytes=wbytes,
                    tb_per_s=round(wbytes / w_ms / 1e9, 3), frac_of_6_29=round(wbytes / w_ms / 1e9 / HBM_TBS, 3), of_decode=round(w_ms / dec_ms, 3),
                    first_row_matches_numpy=wok))
    res.append(dict(summary="stats + windows over decode", ratio=round((st_ms + w_ms) / dec_ms, 3)))
    text = "\n".join(json.dumps(r) for r in res)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
