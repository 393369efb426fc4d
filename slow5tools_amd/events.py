"""events: scrappie-style event segmentation of decoded reads, made on the device where the decoder left them
(include/slow5gpu.h "events", docs/codecs.md §4.15).

A read is cut at the peaks of two sliding t-tests (windows w1 < w2) found by a small peak detector; every event is a row
start | length | mean | stdv.  The t-statistic is computed on the raw integers, so the cut points are reproducible bit for bit.

  events_dev  : a DecodedDev -> (rows, first) on the device: the count pass, a scan and the fill pass; no sample leaves the device
  read_events : records -> (EVENT array, first, status) through s5gpu_signal_events_batch: compressed bytes go up, 16 bytes per event come back
  file_events : a .blow5 file -> (ids, list of EVENT arrays) through the s5events tool

There is no host implementation of the detector here: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from ._lib import NORM_PA, NORM_RAW, REC_ZLIB, SIG_SVB_ZD, EventParams, check

# numpy mirror of s5gpu_event_t (include/slow5gpu.h)
EVENT = np.dtype([("start", "<u4"), ("length", "<u4"), ("mean", "<f4"), ("stdv", "<f4")])
assert EVENT.itemsize == 16

# (w1, w2, thr1, thr2, peak_height): scrappie's defaults for DNA and its RNA preset
DNA = (3, 6, 1.4, 9.0, 0.2)
RNA = (7, 14, 2.5, 9.0, 1.0)
MODES = {"raw": NORM_RAW, "pa": NORM_PA}
S5EVENTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5events")


def _params(params):
    w1, w2, thr1, thr2, ph = params
    return EventParams(int(w1), int(w2), float(thr1), float(thr2), float(ph))


def _mode(mode):
    if mode not in MODES:
        raise ValueError("events: mode must be 'raw' or 'pa', not %r" % (mode,))
    return MODES[mode]


def events_dev(dec, params=DNA, mode="raw"):
    """k_sig_events on what press.decode_to_device left on the device -> (rows, first): rows an [E, 4] int32 tensor on the device (columns
    start, length, and the float32 bits of mean and stdv: rows[:, 2:].view(torch.float32)), first the [n + 1] int64 prefix (the rows of read i
    are rows[first[i]:first[i + 1]]; a record that failed to decode has none).  Only the total row count comes to the host, to size `rows`."""
    import torch

    L = _lib.lib()
    p, m, n = _params(params), _mode(mode), dec.n
    t_off = torch.from_numpy(dec.sig_off.astype(np.uint64).view(np.int64)).to(dec.dev)
    t_cap = torch.from_numpy(dec.sig_cap.astype(np.uint32).view(np.int32)).to(dec.dev)
    t_cnt = torch.zeros(max(n, 1), dtype=torch.int32, device=dec.dev)
    t_st = torch.zeros(max(n, 1), dtype=torch.int32, device=dec.dev)
    st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
    check(L.s5gpu_signal_events_dev(n, dec.t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), dec.t_fields.data_ptr(), C.byref(p), m,
                                    None, None, None, t_cnt.data_ptr(), t_st.data_ptr(), st), "s5gpu_signal_events_dev (count)")
    first = torch.zeros(n + 1, dtype=torch.int64, device=dec.dev)
    if n:
        first[1:] = torch.cumsum(t_cnt[:n].to(torch.int64), 0)
    total = int(first[n].item())
    rows = torch.zeros((total, 4), dtype=torch.int32, device=dec.dev)
    if total:
        check(L.s5gpu_signal_events_dev(n, dec.t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), dec.t_fields.data_ptr(), C.byref(p), m,
                                        first.data_ptr(), t_cnt.data_ptr(), rows.data_ptr(), t_cnt.data_ptr(), t_st.data_ptr(), st),
              "s5gpu_signal_events_dev (fill)")
    torch.cuda.synchronize(dec.dev)
    return rows, first


def read_events(records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, params=DNA, mode="raw", raise_on_error=True):
    """Events of a batch of records (bytes without the u64 prefix) through s5gpu_signal_events_batch -> (events, first, status): an EVENT
    array, the [n + 1] uint64 prefix and the decoder's statuses.  A corrupt record raises; with raise_on_error=False it has its status and
    no events, the other reads' events are valid."""
    L = _lib.lib()
    p, m, n = _params(params), _mode(mode), len(records)
    first = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    vp = C.c_void_p
    rb = [bytes(r) for r in records]
    rbuf = [C.create_string_buffer(r, max(len(r), 1)) for r in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(r) for r in rb])
    rows = np.zeros(max(sum(len(r) for r in rb) // 16, 64), dtype=EVENT)
    for _ in range(2):
        rc = L.s5gpu_signal_events_batch(n, rec_p, rl, rec_method, sig_method, C.byref(p), m, rows.ctypes.data_as(vp), len(rows),
                                         first.ctypes.data_as(vp), status.ctypes.data_as(vp))
        if rc != -3:
            break
        rows = np.zeros(int(first[0]), dtype=EVENT)                        # S5GPU_ERR_NOMEM: first[0] = the rows needed
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_signal_events_batch")
    return rows[:int(first[n])].copy(), first, status


def file_events(path, batch=4096, rna=False, pa=False):
    """(ids, events) of a .blow5 file, the reads in file order: ids a list of bytes, events a list of EVENT arrays whose mean and stdv are
    what the tool printed (%.6g).  Runs the s5events tool (examples/s5events.c), `batch` records per device call."""
    if not os.path.exists(S5EVENTS):
        _build.build()
    cmd = [S5EVENTS, "-K", str(int(batch))] + (["--rna"] if rna else []) + (["--pa"] if pa else []) + [os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0:
        raise _lib.S5GpuError("s5events %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    ids, per = [], []
    for ln in p.stdout.split(b"\n"):
        if not ln:
            continue
        rid, _k, s, e, mean, stdv = ln.split(b"\t")
        if not ids or ids[-1] != rid:
            ids.append(rid)
            per.append([])
        per[-1].append((int(s), int(e) - int(s), float(mean), float(stdv)))
    return ids, [np.array(v, dtype=EVENT) for v in per]
