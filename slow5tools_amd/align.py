"""align: which reference positions each event of a read landed on — the whole path of the read's sDTW alignment (map.py), walked back on
the device (include/slow5gpu.h "align", docs/codecs.md §4.17).

A path is monotone, so it is two int32 values per query row i: lo[i] <= hi[i], the first and last reference column event skip + i is
aligned to; lo[0] = start and hi[qlen - 1] = end of the read's MAP_ROW.  lo and hi are [n, qpitch] matrices, -1 behind qlen and in every row
of a read without a path.  Everything is integer and reproducible bit for bit.

  path_dev   : queries, qlen, a reference and the rows of map.sdtw_dev(want_start=True), all on the device -> (lo, hi, status) on the device
  align_dev  : a DecodedDev -> (MAP_ROW array, lo, hi, status) on the host: events, queries, sDTW, paths
  read_align : records -> (MAP_ROW array, lo, hi, events, status) through s5gpu_align_batch: compressed bytes go up, one download comes back
  file_align : a .blow5 file and a reference file -> (ids, one ALIGN_LINE array per read) through the s5align tool

status: 0, map's QUERY_SHORT or the decoder's, STATUS_PATH_WIDE (the span end - start + 1 is above wmax: no path; wmax bounds the scratch,
not the quality) or STATUS_PATH_ROW (the row is unusable, for one made without want_start).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from . import events as _events
from . import map as _map
from ._lib import REC_ZLIB, SIG_SVB_ZD, STATUS_PATH_ROW, STATUS_PATH_WIDE, check  # noqa: F401  (the statuses: for callers)
from .events import DNA, RNA  # noqa: F401  (RNA: for callers)
from .map import CLIP, MAP_ROW, QMAX, QMIN, SCALE, SKIP

# numpy mirror of s5gpu_event_t, and a line of the tool
EVENT = np.dtype([("start", "<u4"), ("length", "<u4"), ("mean", "<f4"), ("stdv", "<f4")])
ALIGN_LINE = np.dtype([("event", "<i8"), ("sample_start", "<i8"), ("sample_end", "<i8"), ("mean", "<f8"), ("lo", "<i4"), ("hi", "<i4")])
WMAX = 1 << 20
S5ALIGN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5align")


def slot_bytes(qpitch, wmax):
    """the scratch one read needs in path_dev (0: a pitch or wmax it refuses)"""
    return int(_lib.lib().s5gpu_sdtw_path_slot_bytes(int(qpitch), int(wmax)))


def path_dev(queries, qlen, ref_tensor, rows, wmax=None, scratch_bytes=None):
    """k_sdtw_dirs and k_sdtw_trace: queries [n, qpitch] int16, qlen [n] int32, ref_tensor [R] int16 and rows [n, 4] int32 (what
    map.sdtw_dev(..., want_start=True) returned), all on one device -> (lo, hi, status): [n, qpitch] int32 twice and [n] int32 on that
    device.  wmax=None: 4 qpitch.  scratch_bytes=None: a slot for every read, at most 1 GiB (reads then go in groups).  Asynchronous, on
    the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 2 or ref_tensor.dim() != 1:
        raise ValueError("path_dev: queries [n, qpitch] and ref_tensor [R] are int16 tensors")
    if rows.dtype != torch.int32 or tuple(rows.shape) != (int(queries.shape[0]), 4):
        raise ValueError("path_dev: rows is the [n, 4] int32 tensor of sdtw_dev")
    queries, ref_tensor, qlen, rows = queries.contiguous(), ref_tensor.contiguous(), qlen.to(torch.int32).contiguous(), rows.contiguous()
    n, pitch, dev = int(queries.shape[0]), int(queries.shape[1]), queries.device
    wmax = 4 * pitch if wmax is None else int(wmax)
    slot = slot_bytes(pitch, wmax)
    if scratch_bytes is None:
        scratch_bytes = max(slot, min(slot * max(n, 1), 1 << 30))
    scratch = torch.empty(max(int(scratch_bytes), 16) // 4 + 4, dtype=torch.int32, device=dev)
    lo = torch.zeros((max(n, 1), pitch), dtype=torch.int32, device=dev)
    hi = torch.zeros((max(n, 1), pitch), dtype=torch.int32, device=dev)
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_sdtw_path_dev(n, queries.data_ptr(), pitch, qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                         int(ref_tensor.numel()), rows.data_ptr(), wmax, scratch.data_ptr(), int(scratch_bytes), lo.data_ptr(), hi.data_ptr(),
                                         st.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_sdtw_path_dev")
    return lo[:n], hi[:n], st[:n]


def align_dev(dec, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, wmax=None, scratch_bytes=None):
    """events, queries, sDTW and paths on what press.decode_to_device left on the device -> (MAP_ROW array, lo, hi, status) on the host.
    ref: the quantised reference, an int16 numpy array or a device tensor.  status: the query's where that is not 0, else the path's."""
    import torch

    rows, first = _events.events_dev(dec, event_params, "raw")
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()          # s5gpu_rec_fields_t.status
    q, ql, st = _map.queries_dev(rows, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    out = _map.sdtw_dev(q, ql, r, True)
    lo, hi, pst = path_dev(q, ql, r, out, wmax, scratch_bytes)
    st = torch.where(st != 0, st, pst)
    return out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), lo.cpu().numpy().copy(), hi.cpu().numpy().copy(), st.cpu().numpy().copy()


def read_align(records, ref, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
               wmax=None, raise_on_error=True):
    """A batch of records (bytes without the u64 prefix) against the quantised reference `ref` (int16) through s5gpu_align_batch ->
    (MAP_ROW array, lo, hi, events, status): lo, hi [n, qmax] int32, events an [n, qmax] EVENT array (the query's own event rows, zeros
    behind qlen).  A corrupt record raises; with raise_on_error=False it has its status and empty outputs, the others are valid."""
    L = _lib.lib()
    n = len(records)
    ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
    r = np.ascontiguousarray(ref, dtype=np.int16)
    vp = C.c_void_p
    rb = [bytes(x) for x in records]
    rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
    rows = np.zeros(n, dtype=MAP_ROW)
    lo, hi = np.zeros((n, int(qmax)), dtype=np.int32), np.zeros((n, int(qmax)), dtype=np.int32)
    ev = np.zeros((n, int(qmax)), dtype=EVENT)
    status = np.zeros(n, dtype=np.int32)
    rc = L.s5gpu_align_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), 4 * int(qmax) if wmax is None else int(wmax),
                             r.ctypes.data_as(vp), len(r), rows.ctypes.data_as(vp), lo.ctypes.data_as(vp), hi.ctypes.data_as(vp), ev.ctypes.data_as(vp),
                             status.ctypes.data_as(vp))
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_align_batch")
    return rows, lo, hi, ev, status


def file_align(path, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, wmax=None, raise_on_corrupt=True):
    """(ids, lines) of a .blow5 file against the levels of ref_path (one number per line), the reads in file order: ids a list of bytes,
    lines one ALIGN_LINE array per read, a row per query event (empty: the read has no path).  Runs the s5align tool (examples/s5align.c),
    `batch` records per device call.  A corrupt record raises; with raise_on_corrupt=False it is left out."""
    if not os.path.exists(S5ALIGN):
        _build.build()
    cmd = [S5ALIGN, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin))]
    cmd += (["--rna"] if rna else []) + (["--max-span", str(int(wmax))] if wmax is not None else []) + [os.fspath(ref_path), os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5align %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    ids, lines = [], []
    for ln in p.stdout.split(b"\n"):
        if not ln:
            continue
        f = ln.split(b"\t")
        if f[1] == b"*" or int(f[1]) == int(skip):                         # a read's first line: no path, or its first query event
            ids.append(f[0])
            lines.append([])
        if f[1] != b"*":
            lines[-1].append((int(f[1]), int(f[2]), int(f[3]), float(f[4]), int(f[5]), int(f[6])))
    return ids, [np.array(l, dtype=ALIGN_LINE).reshape(-1) for l in lines]
