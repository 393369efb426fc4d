"""map: where in a target each read came from — subsequence DTW of the read's events against a reference squiggle, on the device
(include/slow5gpu.h "map", docs/codecs.md §4.16).

A read's query is the quantised means of its event rows [skip, skip + qlen); the reference is a sequence of expected current levels that the
caller brings (no pore model ships with this project), quantised the same way.  From the quantiser onward everything is integer: cost, end and
start are reproducible bit for bit.

  quantise    : float32 values -> int16, on the host (the reference)
  queries_dev : event rows + prefix on the device -> (queries [n, qmax] int16, qlen, status) on the device
  sdtw_dev    : queries, qlen and a reference on the device -> [n, 4] int32 rows cost | qlen | start | end on the device
  map_dev     : a DecodedDev -> (MAP_ROW array, status): events, queries, sDTW; only the 16 n result bytes (and the statuses) leave the device
  read_map    : records -> (MAP_ROW array, status) through s5gpu_map_batch: compressed bytes go up, 16 bytes per read come back
  file_map    : a .blow5 file and a reference file -> (ids, MAP_ROW array) through the s5map tool

There is no host implementation of the alignment here: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from . import events as _events
from ._lib import REC_ZLIB, SIG_SVB_ZD, STATUS_QUERY_SHORT, MapParams, check  # noqa: F401  (STATUS_QUERY_SHORT: for callers)
from .events import DNA, RNA  # noqa: F401  (RNA: for callers)

# numpy mirror of s5gpu_map_row_t (include/slow5gpu.h)
MAP_ROW = np.dtype([("cost", "<u4"), ("qlen", "<u4"), ("start", "<i4"), ("end", "<i4")])
assert MAP_ROW.itemsize == 16
NO_COST = 0xFFFFFFFF
SCALE, CLIP = 32.0, 127
# the tool's defaults: event rows left out in front, rows of the query at most, rows a read needs
SKIP, QMAX, QMIN = 0, 250, 50
S5MAP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5map")


def _params(skip, qmax, qmin, scale, clip, want_start):
    return MapParams(int(skip), int(qmax), int(qmin), float(scale), int(clip), 1 if want_start else 0)


def quantise(means, scale=SCALE, clip=CLIP):
    """quant of §4.16 on the host (s5gpu_quantise_host): float32 values -> int16 of mean 0 and standard deviation `scale`, clipped at +-clip"""
    m = np.ascontiguousarray(means, dtype=np.float32)
    if m.ndim != 1:
        raise ValueError("quantise: a one-dimensional array of values")
    q = np.zeros(len(m), dtype=np.int16)
    check(_lib.lib().s5gpu_quantise_host(m.ctypes.data_as(C.c_void_p), len(m), float(scale), int(clip), q.ctypes.data_as(C.c_void_p)), "s5gpu_quantise_host")
    return q


def queries_dev(rows, first, status=None, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP):
    """k_ev_query on what events.events_dev returned -> (queries, qlen, status) on the device: queries an [n, qmax] int16 tensor (row i the
    query of read i, zeros behind qlen[i]), qlen and status [n] int32.  status (optional): the [n] int32 statuses of the reads (a failed
    record's wins and it has no query)."""
    import torch

    n = int(first.numel()) - 1
    dev = first.device
    p = _params(skip, qmax, qmin, scale, clip, False)
    q = torch.zeros((max(n, 1), int(qmax)), dtype=torch.int16, device=dev)
    ql = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    rows = rows.contiguous()
    first = first.contiguous()
    if status is not None:
        status = status.to(torch.int32).contiguous()
    check(_lib.lib().s5gpu_event_queries_dev(n, rows.data_ptr() if rows.numel() else None, first.data_ptr(), status.data_ptr() if status is not None else None,
                                             C.byref(p), q.data_ptr(), ql.data_ptr(), st.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          "s5gpu_event_queries_dev")
    return q[:n], ql[:n], st[:n]


def sdtw_dev(queries, qlen, ref_tensor, want_start=False):
    """k_sdtw: queries [n, qpitch] int16, qlen [n] int32 and ref_tensor [R] int16, all on one device -> an [n, 4] int32 tensor on that device,
    columns cost (as uint32 bits), qlen, start (-1 unless want_start), end.  Asynchronous, on the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 2 or ref_tensor.dim() != 1:
        raise ValueError("sdtw_dev: queries [n, qpitch] and ref_tensor [R] are int16 tensors")
    queries, ref_tensor, qlen = queries.contiguous(), ref_tensor.contiguous(), qlen.to(torch.int32).contiguous()
    n, dev = int(queries.shape[0]), queries.device
    out = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_sdtw_dev(n, queries.data_ptr(), int(queries.shape[1]), qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                    int(ref_tensor.numel()), 1 if want_start else 0, out.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
          "s5gpu_sdtw_dev")
    return out[:n]


def map_dev(dec, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, want_start=False):
    """events, queries and sDTW on what press.decode_to_device left on the device -> (MAP_ROW array, status) on the host.  ref: the quantised
    reference, an int16 numpy array or a device tensor.  Only the 16 n result bytes and the n statuses leave the device."""
    import torch

    rows, first = _events.events_dev(dec, event_params, "raw")
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()          # s5gpu_rec_fields_t.status
    q, ql, st = queries_dev(rows, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    out = sdtw_dev(q, ql, r.to(dec.dev), want_start)
    return out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), st.cpu().numpy().copy()


def read_map(records, ref, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
             want_start=False, raise_on_error=True):
    """A batch of records (bytes without the u64 prefix) against the quantised reference `ref` (int16) through s5gpu_map_batch ->
    (MAP_ROW array, status).  A corrupt record raises; with raise_on_error=False it has its status and the empty row, the others are valid."""
    L = _lib.lib()
    n = len(records)
    ep, mp = _events._params(event_params), _params(skip, qmax, qmin, scale, clip, want_start)
    r = np.ascontiguousarray(ref, dtype=np.int16)
    vp = C.c_void_p
    rb = [bytes(x) for x in records]
    rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
    rows = np.zeros(n, dtype=MAP_ROW)
    status = np.zeros(n, dtype=np.int32)
    rc = L.s5gpu_map_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), r.ctypes.data_as(vp), len(r), rows.ctypes.data_as(vp),
                           status.ctypes.data_as(vp))
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_map_batch")
    return rows, status


def file_map(path, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, want_start=False):
    """(ids, rows) of a .blow5 file against the levels of ref_path (one number per line), the reads in file order: ids a list of bytes, rows a
    MAP_ROW array (a read whose query is too short: the empty row).  Runs the s5map tool (examples/s5map.c), `batch` records per device call."""
    if not os.path.exists(S5MAP):
        _build.build()
    cmd = [S5MAP, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin))]
    cmd += (["--rna"] if rna else []) + (["--start"] if want_start else []) + [os.fspath(ref_path), os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0:
        raise _lib.S5GpuError("s5map %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    ids, rows = [], []
    for ln in p.stdout.split(b"\n"):
        if not ln:
            continue
        rid, used, cost, _per, start, end = ln.split(b"\t")
        ids.append(rid)
        rows.append((NO_COST, 0, -1, -1) if used == b"*" else (int(cost), int(used), -1 if start == b"*" else int(start), int(end)))
    return ids, np.array(rows, dtype=MAP_ROW).reshape(-1)
