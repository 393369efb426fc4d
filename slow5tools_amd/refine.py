"""refine: per-read level rescaling from the path, and a windowed realign (include/slow5gpu.h "refine", docs/codecs.md §4.20).

A read's query and the reference are normalised apart (map.py).  refine fits the line r = a q + b over the cells of the read's path
(align.py), requantises the query with it and aligns it again in a window of the reference around the first hit, `iters` times, each round
from the query that came in and along the path of the round before.  The reference is left as it is, so costs before and after compare.
Sums are exact integers and the solve is pinned in double: everything is reproducible bit for bit.

  fit_dev     : queries, qlen, a reference, lo, hi and status as align.path_dev left them -> (FIT tensor, q', status) on the device
  window_dev  : queries, qlen, a reference and rows -> (rows', lo, hi, status) on the device: sDTW and its path inside [start - pad, end + pad]
  refine_dev  : the rounds of the two on the device -> Refined(queries, rows, lo, hi, fit, status, rounds), which feeds pileup.accum_dev as it is
  refine_on   : a DecodedDev -> (MAP_ROW array of the first mapping, Refined on the host)
  read_refine : records -> (rows, rows_refined, FIT array, lo, hi, events, status, rounds) through s5gpu_refine_batch
  file_refine : a .blow5 file and a reference file -> (ids, REFINE_LINE array) through the s5refine tool

status: what align gives, or STATUS_FIT_FLAT (too few cells, or a query without variance along the path), STATUS_FIT_RANGE (the slope or the
shift is outside what RefineParams accepts), STATUS_PATH_WIDE (the window is above wmax); a read with one of these three keeps the result
of the last round that succeeded (none: what came in).  The defaults of RefineParams come from a prototype; they are not tuned on data.
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import align as _align
from . import build as _build
from . import events as _events
from . import map as _map
from ._lib import REC_ZLIB, SIG_SVB_ZD, STATUS_FIT_FLAT, STATUS_FIT_RANGE, STATUS_PATH_ROW, STATUS_PATH_WIDE, check  # noqa: F401  (for callers)
from .events import DNA, RNA  # noqa: F401  (RNA: for callers)
from .map import CLIP, MAP_ROW, QMAX, QMIN, SCALE, SKIP

FIT = _lib.Fit
EVENT = _align.EVENT
# a line of the tool (cost -1, the columns -1 and scale / shift nan: `*`)
REFINE_LINE = np.dtype([("events_used", "<i8"), ("cost", "<i8"), ("ref_start", "<i8"), ("ref_end", "<i8"), ("scale", "<f8"), ("shift", "<f8"), ("rounds", "<i8"),
                        ("cost_refined", "<i8"), ("ref_start_refined", "<i8"), ("ref_end_refined", "<i8"), ("fit", "S8")])
S5REFINE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5refine")
Refined = collections.namedtuple("Refined", "queries rows lo hi fit status rounds")


def RefineParams(a_min=0.5, a_max=2.0, b_max=64.0, clip=CLIP, pad=16, min_cells=16, iters=2):
    """s5gpu_refine_params_t: slopes in [a_min, a_max] and |shift| <= b_max are accepted, q' is clamped to +-clip, the window is the row's
    span and `pad` columns either side, a fit needs min_cells cells, refine_dev makes `iters` rounds"""
    return _lib.RefineParams(float(a_min), float(a_max), float(b_max), int(clip), int(pad), int(min_cells), int(iters))


def _check_inputs(who, queries, ref_tensor):
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 2 or ref_tensor.dim() != 1:
        raise ValueError("%s: queries [n, qpitch] and ref_tensor [R] are int16 tensors" % who)


def _scratch(n, pitch, wmax, scratch_bytes, dev):
    import torch

    slot = _align.slot_bytes(pitch, wmax)
    if scratch_bytes is None:
        scratch_bytes = max(slot, min(slot * max(n, 1), 1 << 30))
    return torch.empty(max(int(scratch_bytes), 16) // 4 + 4, dtype=torch.int32, device=dev), int(scratch_bytes)


def fit_dev(queries, qlen, ref_tensor, lo, hi, status, wmax=None, params=None, want_queries=True):
    """k_path_fit -> (fit, queries', status'): fit an [n, 8] int64 tensor whose rows are FIT records (a and b are the doubles behind its first
    two columns: fit.cpu().numpy().view(FIT)), queries' [n, qpitch] int16 (None without want_queries), status' [n] int32.  wmax=None:
    4 qpitch.  Asynchronous, on the current stream."""
    import torch

    _check_inputs("fit_dev", queries, ref_tensor)
    n, pitch, dev = int(queries.shape[0]), int(queries.shape[1]), queries.device
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (n, pitch) or tuple(hi.shape) != (n, pitch):
        raise ValueError("fit_dev: lo and hi are [n, qpitch] int32 tensors")
    queries, ref_tensor, lo, hi = queries.contiguous(), ref_tensor.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    p = params if params is not None else RefineParams()
    fit = torch.zeros((max(n, 1), 8), dtype=torch.int64, device=dev)
    qo = torch.zeros((max(n, 1), pitch), dtype=torch.int16, device=dev) if want_queries else None
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_path_fit_dev(n, queries.data_ptr(), pitch, qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                        int(ref_tensor.numel()), lo.data_ptr(), hi.data_ptr(), status.data_ptr(), 4 * pitch if wmax is None else int(wmax),
                                        C.byref(p), fit.data_ptr(), qo.data_ptr() if qo is not None else None, st.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_path_fit_dev")
    for t in (queries, ref_tensor, lo, hi, qlen, status):                  # (copies made here die with this frame)
        t.record_stream(torch.cuda.current_stream(dev))
    return fit[:n], (qo[:n] if qo is not None else None), st[:n]


def window_dev(queries, qlen, ref_tensor, rows, pad=16, wmax=None, scratch_bytes=None):
    """k_sdtw_win and k_sdtw_trace_win -> (rows', lo, hi, status): rows' [n, 4] int32 (cost', qlen, start', end'), lo and hi [n, qpitch]
    int32, status [n] int32, the alignment of each query inside [start - pad, end + pad] of its row in `rows` ([n, 4] int32).  wmax=None:
    4 qpitch + 2 pad.  Asynchronous, on the current stream."""
    import torch

    _check_inputs("window_dev", queries, ref_tensor)
    n, pitch, dev = int(queries.shape[0]), int(queries.shape[1]), queries.device
    if rows.dtype != torch.int32 or tuple(rows.shape) != (n, 4):
        raise ValueError("window_dev: rows is an [n, 4] int32 tensor")
    queries, ref_tensor, qlen, rows = queries.contiguous(), ref_tensor.contiguous(), qlen.to(torch.int32).contiguous(), rows.contiguous()
    wmax = min(4 * pitch + 2 * int(pad), _align.WMAX) if wmax is None else int(wmax)
    scratch, sb = _scratch(n, pitch, wmax, scratch_bytes, dev)
    out = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    lo = torch.zeros((max(n, 1), pitch), dtype=torch.int32, device=dev)
    hi = torch.zeros((max(n, 1), pitch), dtype=torch.int32, device=dev)
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_sdtw_window_dev(n, queries.data_ptr(), pitch, qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                           int(ref_tensor.numel()), rows.data_ptr(), int(pad), wmax, scratch.data_ptr(), sb, out.data_ptr(), lo.data_ptr(),
                                           hi.data_ptr(), st.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_sdtw_window_dev")
    for t in (queries, ref_tensor, qlen, rows, scratch):
        t.record_stream(torch.cuda.current_stream(dev))
    return out[:n], lo[:n], hi[:n], st[:n]


def refine_dev(queries, qlen, ref_tensor, rows, lo, hi, status, wmax=None, params=None, scratch_bytes=None):
    """s5gpu_refine_dev on what map.sdtw_dev(want_start=True) and align.path_dev left on the device -> Refined(queries, rows, lo, hi, fit,
    status, rounds), all on the device: queries [n, qpitch] int16, rows [n, 4] int32, lo and hi [n, qpitch] int32, fit [n, 8] int64 (FIT
    records), status [n] int32, rounds [n] int32.  wmax=None: 4 qpitch + 2 pad.  Asynchronous, on the current stream."""
    import torch

    _check_inputs("refine_dev", queries, ref_tensor)
    n, pitch, dev = int(queries.shape[0]), int(queries.shape[1]), queries.device
    if rows.dtype != torch.int32 or tuple(rows.shape) != (n, 4):
        raise ValueError("refine_dev: rows is the [n, 4] int32 tensor of sdtw_dev")
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (n, pitch) or tuple(hi.shape) != (n, pitch):
        raise ValueError("refine_dev: lo and hi are [n, qpitch] int32 tensors")
    queries, ref_tensor, rows, lo, hi = queries.contiguous(), ref_tensor.contiguous(), rows.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    p = params if params is not None else RefineParams()
    wmax = min(4 * pitch + 2 * int(p.pad), _align.WMAX) if wmax is None else int(wmax)
    scratch, sb = _scratch(n, pitch, wmax, scratch_bytes, dev)
    wb = int(_lib.lib().s5gpu_refine_work_bytes(n, pitch))
    work = torch.empty(max(wb, 16) // 8 + 2, dtype=torch.int64, device=dev)
    m = max(n, 1)
    qo = torch.zeros((m, pitch), dtype=torch.int16, device=dev)
    ro = torch.zeros((m, 4), dtype=torch.int32, device=dev)
    lo2, hi2 = torch.zeros((m, pitch), dtype=torch.int32, device=dev), torch.zeros((m, pitch), dtype=torch.int32, device=dev)
    fit = torch.zeros((m, 8), dtype=torch.int64, device=dev)
    st, rounds = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_refine_dev(n, queries.data_ptr(), pitch, qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                      int(ref_tensor.numel()), rows.data_ptr(), lo.data_ptr(), hi.data_ptr(), status.data_ptr(), wmax, C.byref(p),
                                      scratch.data_ptr(), sb, work.data_ptr(), wb, qo.data_ptr(), ro.data_ptr(), lo2.data_ptr(), hi2.data_ptr(), fit.data_ptr(),
                                      st.data_ptr(), rounds.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_refine_dev")
    for t in (queries, ref_tensor, rows, lo, hi, qlen, status, scratch, work):
        t.record_stream(torch.cuda.current_stream(dev))
    return Refined(qo[:n], ro[:n], lo2[:n], hi2[:n], fit[:n], st[:n], rounds[:n])


def refine_on(dec, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, wmax=None, params=None, scratch_bytes=None, host=True):
    """events, queries, sDTW, paths and the rounds on what press.decode_to_device left on the device -> (MAP_ROW array of the first mapping,
    Refined).  host=True: Refined holds numpy arrays (rows a MAP_ROW array, fit a FIT array); False: the device tensors of refine_dev, and
    the first rows as an [n, 4] int32 tensor.  ref: the quantised reference, an int16 numpy array or a device tensor.  wmax=None: 4 qmax."""
    import torch

    ev, first = _events.events_dev(dec, event_params, "raw")
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()          # s5gpu_rec_fields_t.status
    q, ql, st = _map.queries_dev(ev, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    wmax = 4 * int(qmax) if wmax is None else int(wmax)
    out = _map.sdtw_dev(q, ql, r, True)
    lo, hi, pst = _align.path_dev(q, ql, r, out, wmax, scratch_bytes)
    st = torch.where(st != 0, st, pst)
    R = refine_dev(q, ql, r, out, lo, hi, st, wmax, params, scratch_bytes)
    if not host:
        return out, R
    return out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), Refined(R.queries.cpu().numpy(), R.rows.cpu().numpy().view(MAP_ROW).reshape(-1).copy(),
                                                                       R.lo.cpu().numpy(), R.hi.cpu().numpy(), R.fit.cpu().numpy().view(FIT).reshape(-1).copy(),
                                                                       R.status.cpu().numpy(), R.rounds.cpu().numpy())


def read_refine(records, ref, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
                wmax=None, params=None, raise_on_error=True):
    """A batch of records (bytes without the u64 prefix) against the quantised reference `ref` (int16) through s5gpu_refine_batch ->
    (rows, rows_refined, fit, lo, hi, events, status, rounds): two MAP_ROW arrays, a FIT array, the refined path as [n, qmax] int32 twice, an
    [n, qmax] EVENT array, [n] int32 twice.  A corrupt record raises; with raise_on_error=False it has its status and empty outputs."""
    L = _lib.lib()
    n = len(records)
    ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
    p = params if params is not None else RefineParams()
    r = np.ascontiguousarray(ref, dtype=np.int16)
    vp = C.c_void_p
    rb = [bytes(x) for x in records]
    rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
    rows, rows2, fit = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=FIT)
    lo, hi = np.zeros((n, int(qmax)), dtype=np.int32), np.zeros((n, int(qmax)), dtype=np.int32)
    ev = np.zeros((n, int(qmax)), dtype=EVENT)
    status, rounds = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    rc = L.s5gpu_refine_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), 4 * int(qmax) if wmax is None else int(wmax), C.byref(p),
                              r.ctypes.data_as(vp), len(r), rows.ctypes.data_as(vp), rows2.ctypes.data_as(vp), fit.ctypes.data_as(vp), lo.ctypes.data_as(vp),
                              hi.ctypes.data_as(vp), ev.ctypes.data_as(vp), status.ctypes.data_as(vp), rounds.ctypes.data_as(vp))
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_refine_batch")
    return rows, rows2, fit, lo, hi, ev, status, rounds


def file_refine(path, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, wmax=None, pad=None, iters=None, slope=None, raise_on_corrupt=True):
    """(ids, lines) of a .blow5 file against the levels of ref_path (one number per line), the reads in file order: ids a list of bytes,
    lines a REFINE_LINE array.  Runs the s5refine tool (examples/s5refine.c), `batch` records per device call.  A corrupt record raises;
    with raise_on_corrupt=False it is left out."""
    if not os.path.exists(S5REFINE):
        _build.build()
    cmd = [S5REFINE, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin))]
    cmd += (["--rna"] if rna else []) + (["--max-span", str(int(wmax))] if wmax is not None else [])
    cmd += (["--pad", str(int(pad))] if pad is not None else []) + (["--iters", str(int(iters))] if iters is not None else [])
    cmd += (["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []) + [os.fspath(ref_path), os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5refine %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    ids, lines = [], []

    def num(x, f=int, none=-1):
        return none if x == b"*" else f(x)
    for ln in p.stdout.split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            ids.append(f[0])
            lines.append((num(f[1]), num(f[2]), num(f[3]), num(f[4]), num(f[5], float, np.nan), num(f[6], float, np.nan), num(f[7]), num(f[8]), num(f[9]),
                          num(f[10]), f[11]))
    return ids, np.array(lines, dtype=REFINE_LINE).reshape(-1)
