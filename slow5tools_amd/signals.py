"""Signals for a consumer: per-read order statistics and normalised windows of decoded reads, made on the device
(include/slow5gpu.h "signals", docs/codecs.md §4.11).

  chunk_plan    : how a read of T samples is cut into windows of W samples (pure numpy; the rule is this project's own)
  signal_stats  : records -> statistics through s5gpu_signal_stats_stream (the signals never leave the device)
  read_signals  : records -> a dense [n_windows, W] tensor of normalised samples on the device
"""
import ctypes as C
import struct

import numpy as np

from . import _lib, press
from ._lib import NORM_MEDMAD, NORM_PA, NORM_QUANT, NORM_RAW, REC_ZLIB, SIG_F16, SIG_F32, SIG_SVB_ZD, check

# numpy mirror of s5gpu_sig_stats_t (include/slow5gpu.h)
SIG_STATS = np.dtype([("n", "<u4"), ("status", "<i4"), ("sum", "<i8"), ("sumsq", "<u8"), ("med2", "<i4"), ("mad4", "<u4"),
                      ("min", "<i2"), ("max", "<i2"), ("q", "<i2", (4,)), ("reserved", "<u4")])
assert SIG_STATS.itemsize == 48

NORMS = {"raw": NORM_RAW, "pa": NORM_PA, "medmad": NORM_MEDMAD, "quant": NORM_QUANT}


def chunk_plan(n_samples, window, overlap=0):
    """Windows of `window` samples over reads of n_samples[i] samples -> (win_read, win_start), uint32 arrays, the reads in order.
    A read of T samples: T = 0 gives no window; T <= W one window at 0 (its tail is padding); otherwise windows start at
    0, W - overlap, 2 (W - overlap), ... while start + W <= T, and if the last of them does not end at T one more starts at T - W."""
    W, ov = int(window), int(overlap)
    if W <= 0 or ov < 0 or ov >= W:
        raise ValueError("chunk_plan: window %d, overlap %d" % (W, ov))
    T = np.asarray(n_samples, dtype=np.int64).reshape(-1)
    step = W - ov
    k = np.where(T > W, (np.maximum(T, W) - W) // step + 1, (T > 0).astype(np.int64))      # windows on the regular grid
    extra = (T > W) & ((k - 1) * step + W != T)
    cnt = k + extra
    total = int(cnt.sum())
    win_read = np.repeat(np.arange(len(T), dtype=np.int64), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(T) else np.zeros(0, np.int64)
    idx = np.arange(total, dtype=np.int64) - np.repeat(first, cnt)                          # index of a window within its read
    start = idx * step
    last_extra = np.repeat(extra, cnt) & (idx == np.repeat(cnt, cnt) - 1)
    start[last_extra] = np.repeat(T, cnt)[last_extra] - W
    return win_read.astype(np.uint32), start.astype(np.uint32)


def _quantile_array(quantiles):
    q = [float(x) for x in quantiles]
    return len(q), (C.c_double * max(len(q), 1))(*q)


def signal_stats(records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, quantiles=(), raise_on_error=True, with_fields=False):
    """Statistics of a batch of records (bytes without the u64 prefix) through s5gpu_signal_stats_stream: a SIG_STATS array
    (and the REC_FIELDS array with with_fields).  A corrupt record raises, or with raise_on_error=False shows in its status."""
    L = _lib.lib()
    n = len(records)
    stats = np.zeros(n, dtype=SIG_STATS)
    fields = np.zeros(n, dtype=_lib.REC_FIELDS)
    if n:
        pos, parts, at = np.zeros(n, dtype=np.uint64), [], 0
        for i, r in enumerate(records):
            r = bytes(r)
            parts.append(struct.pack("<Q", len(r)) + r)
            pos[i] = at + 8
            at += 8 + len(r)
        chunk = np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8)
        lens = np.array([len(r) for r in records], dtype=np.uint32)
        n_q, q = _quantile_array(quantiles)
        vp = C.c_void_p
        rc = L.s5gpu_signal_stats_stream(n, chunk.ctypes.data_as(vp), at, pos.ctypes.data_as(vp), lens.ctypes.data_as(vp), rec_method, sig_method,
                                         n_q, q, stats.ctypes.data_as(vp), fields.ctypes.data_as(vp))
        if rc != 0 and (raise_on_error or rc != -5):
            check(rc, "s5gpu_signal_stats_stream")
    return (stats, fields) if with_fields else stats


def stats_dev(dec, quantiles=()):
    """k_sig_stats on what press.decode_to_device left on the device -> (stats tensor on the device, 48 bytes per record; sig_off, sig_cap
    tensors the window kernel takes as well)"""
    import torch

    L = _lib.lib()
    t_off = torch.from_numpy(dec.sig_off.astype(np.uint64).view(np.int64)).to(dec.dev)
    t_cap = torch.from_numpy(dec.sig_cap.astype(np.uint32).view(np.int32)).to(dec.dev)
    t_stats = torch.zeros(max(dec.n, 1) * SIG_STATS.itemsize, dtype=torch.uint8, device=dec.dev)
    n_q, q = _quantile_array(quantiles)
    st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
    check(L.s5gpu_signal_stats_dev(dec.n, dec.t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), dec.t_fields.data_ptr(), n_q, q,
                                   t_stats.data_ptr(), st), "s5gpu_signal_stats_dev")
    return t_stats, t_off, t_cap


def read_signals(records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, norm="medmad", window=None, overlap=0, pad_to=None, dtype=None,
                 device="cuda:0", quantiles=(0.2, 0.9), a=0.51, b=0.53):
    """Records (bytes without the u64 prefix) -> (tensor [n_windows, W] on the device, win_read, win_start, stats, fields).
    norm: "raw", "pa" (picoamperes from the read's own fields), "medmad" ((x - median) / (1.4826 MAD)) or "quant"
    ((x - a (q0 + q1)) / max(b (q1 - q0), 1) on the first two of `quantiles`; the defaults are Dorado's q20 / q90 rule).
    window=None: one row per read, padded with zeros to pad_to (default: the longest read).  window=W: chunk_plan(n_samples, W, overlap).
    dtype: torch.float32 (default) or torch.float16.  A record that failed to decode has no window (window=None: a row of zeros);
    stats["status"] says why."""
    import torch

    L = _lib.lib()
    if norm not in NORMS:
        raise ValueError("read_signals: unknown norm %r" % (norm,))
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float16):
        raise ValueError("read_signals: dtype must be torch.float32 or torch.float16")
    n = len(records)
    dec = press.decode_to_device(records, rec_method, sig_method, device=device, no_payload=press.no_payload_methods(rec_method, sig_method))
    t_stats, t_off, t_cap = stats_dev(dec, quantiles)
    fields = dec.t_fields.cpu().numpy().view(_lib.REC_FIELDS)[:n].copy()
    stats = t_stats.cpu().numpy().view(SIG_STATS)[:n].copy()
    n_eff = stats["n"].astype(np.int64)                      # (0 for a record that failed)
    if window is None:
        W = int(pad_to) if pad_to is not None else max(int(n_eff.max()) if n else 0, 1)
        win_read = np.arange(n, dtype=np.uint32)                # row i = read i; the row of a record that failed is zeros
        win_start = np.zeros(n, dtype=np.uint32)
    else:
        W = int(window)
        win_read, win_start = chunk_plan(n_eff, W, overlap)
    nw = len(win_read)
    out = torch.zeros((nw, W), dtype=dtype, device=dec.dev)
    if nw:
        t_wr = torch.from_numpy(win_read.view(np.int32)).to(dec.dev)
        t_ws = torch.from_numpy(win_start.view(np.int32)).to(dec.dev)
        t_wst = torch.zeros(nw, dtype=torch.int32, device=dec.dev)
        st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
        check(L.s5gpu_signal_windows_dev(n, dec.t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), dec.t_fields.data_ptr(), t_stats.data_ptr(),
                                         nw, t_wr.data_ptr(), t_ws.data_ptr(), W, NORMS[norm], float(a), float(b),
                                         SIG_F16 if dtype == torch.float16 else SIG_F32, out.data_ptr(), t_wst.data_ptr(), st),
              "s5gpu_signal_windows_dev")
        torch.cuda.synchronize(dec.dev)
        if not np.array_equal(t_wst.cpu().numpy() != 0, stats["status"][win_read] != 0):
            raise _lib.S5GpuError("read_signals: the device refused windows of the plan made on the host")
    return out, win_read, win_start, stats, fields
