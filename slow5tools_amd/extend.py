"""extend: whole-read banded alignment in tiles from map's anchor (include/slow5gpu.h "extend", docs/codecs.md §4.21).

map, align and refine stop at the first 1024 events of a read.  extend follows the path of all of a read's events from the column where its
prefix mapped: the long query is cut into tiles of `tile_rows` rows, each tile is the sDTW recurrence over a window of `band` reference
columns placed around the column where the tile before ended cheapest, and that tile's last row is carried in.  The cost is
O(events x band) whatever the reference's length.  The band is a heuristic: where the true path leaves it the result is a worse alignment,
not an error; cost / qlen is the only sign.

  queries_long_dev : event rows and their prefix -> (queries, qlen, status) on the device, ragged: read i at queries[first[i]:first[i] + qlen[i]]
  band_dev         : long queries, a reference and an anchor column per read -> (rows, lo, hi) on the device
  fit_long_dev     : long queries, a reference, lo, hi and status as band_dev left them -> (FIT tensor, q', status) on the device (§4.24)
  refine_long_dev  : ... and the rounds of s5gpu_extend_refine_dev -> RefinedLong(queries, rows, lo, hi, fit, rounds) on the device
  extend_dev       : a DecodedDev -> (MAP_ROW array of the prefix mapping, Extended): events, prefix queries, sDTW with the start, long
                     queries, the banded alignment from `start`
  read_extend      : records -> (map_rows, rows, first, lo, hi, events, status) through s5gpu_extend_batch
  file_extend      : a .blow5 file and a reference file -> (ids, EXTEND_LINE array) through the s5extend tool

Layouts are ragged: the query, lo and hi of read i live at [first[i], first[i] + qlen[i]) of arrays as long as the event rows; `first` is the
prefix events.events_dev returns.  The defaults of BandParams come from a prototype; they are not tuned on data.
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
from ._lib import REC_ZLIB, SIG_SVB_ZD, STATUS_PATH_ROW, STATUS_PATH_WIDE, STATUS_QUERY_SHORT, check  # noqa: F401  (for callers)
from .events import DNA, RNA  # noqa: F401  (RNA: for callers)
from .map import CLIP, MAP_ROW, QMAX, QMIN, SCALE, SKIP
from .refine import FIT, RefineParams

EXT_ROW = np.dtype([("cost", "<u8"), ("qlen", "<u4"), ("tiles", "<u4"), ("start", "<i4"), ("end", "<i4"), ("a_last", "<i4"), ("status", "<i4")])
EVENT = _align.EVENT
# a line of the tool (cost -1, cost_per_event nan and the columns -1: `*`)
EXTEND_LINE = np.dtype([("events_used", "<i8"), ("cost", "<i8"), ("cost_per_event", "<f8"), ("ref_start", "<i8"), ("ref_end", "<i8"), ("tiles", "<i8"),
                        ("anchor", "<i8")])
S5EXTEND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5extend")
EMAX = 1 << 20
TILE_ROWS, BAND = 256, 512
Extended = collections.namedtuple("Extended", "rows first queries qlen lo hi")
RefinedLong = collections.namedtuple("RefinedLong", "queries rows lo hi fit rounds")
# what extend_dev returns with refine=...: Extended's fields are the refined ones, rows_first the rows of the first alignment
ExtendedRefined = collections.namedtuple("ExtendedRefined", "rows first queries qlen lo hi rows_first fit rounds")
# the columns s5extend --refine appends to a line (scale and shift nan, the others -1: `*`)
EXTEND_REFINE_LINE = np.dtype(EXTEND_LINE.descr + [("scale", "<f8"), ("shift", "<f8"), ("rounds", "<i8"), ("cost_refined", "<i8"), ("ref_start_refined", "<i8"),
                                                   ("ref_end_refined", "<i8"), ("fit", "S8")])

assert EXT_ROW.itemsize == 32


def BandParams(skip=SKIP, emin=QMIN, emax=EMAX, tile_rows=TILE_ROWS, band=BAND, clip=CLIP, scale=SCALE):
    """s5gpu_band_params_t: event rows [skip, skip + min(emax, E - skip)) make the query, at least emin of them; tiles of tile_rows rows (64,
    128, 256, 512, 1024) over windows of `band` columns (a multiple of 64 in 64 .. 4096); scale and clip as in map"""
    return _lib.BandParams(int(skip), int(emin), int(emax), int(tile_rows), int(band), int(clip), float(scale))


def scratch_bytes(n, total_rows, tile_rows=TILE_ROWS, band=BAND):
    """s5gpu_sdtw_band_scratch_bytes"""
    return int(_lib.lib().s5gpu_sdtw_band_scratch_bytes(int(n), int(total_rows), int(tile_rows), int(band)))


def queries_long_dev(rows, first, status=None, params=None):
    """k_ev_query_long on what events.events_dev returned -> (queries, qlen, status) on the device: queries a [total_rows] int16 tensor (read
    i at first[i], zeros behind qlen[i] up to first[i + 1]), qlen and status [n] int32.  status (optional): the [n] int32 statuses of the
    reads (a failed record's wins and it has no query).  Asynchronous, on the current stream."""
    import torch

    n = int(first.numel()) - 1
    dev = first.device
    p = params if params is not None else BandParams()
    rows, first = rows.contiguous(), first.contiguous()
    total = int(rows.shape[0])
    q = torch.zeros(max(total, 1), dtype=torch.int16, device=dev)
    ql = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    if status is not None:
        status = status.to(torch.int32).contiguous()
    check(_lib.lib().s5gpu_event_queries_long_dev(n, rows.data_ptr() if total else None, first.data_ptr(), status.data_ptr() if status is not None else None,
                                                  C.byref(p), total, q.data_ptr(), ql.data_ptr(), st.data_ptr(),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_event_queries_long_dev")
    for t in (rows, first) + ((status,) if status is not None else ()):
        t.record_stream(torch.cuda.current_stream(dev))
    return q[:total], ql[:n], st[:n]


def band_dev(queries, first, qlen, ref_tensor, anchor, status=None, params=None, scratch_bytes_=None):
    """k_sdtw_band and k_sdtw_band_trace -> (rows, lo, hi): rows an [n, 4] int64 tensor whose rows are EXT_ROW records
    (rows.cpu().numpy().view(EXT_ROW)), lo and hi [total_rows] int32, ragged as the queries.  anchor: [n] int32 columns of ref_tensor ([R]
    int16).  scratch_bytes_ (for tests): the size the call is told instead of what it needs.  Asynchronous, on the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 1 or ref_tensor.dim() != 1:
        raise ValueError("band_dev: queries [total_rows] and ref_tensor [R] are int16 tensors")
    n, total, dev = int(first.numel()) - 1, int(queries.numel()), queries.device
    p = params if params is not None else BandParams()
    queries, first, ref_tensor = queries.contiguous(), first.contiguous(), ref_tensor.contiguous()
    qlen, anchor = qlen.to(torch.int32).contiguous(), anchor.to(torch.int32).contiguous()
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev) if status is None else status.to(torch.int32).contiguous()
    need = scratch_bytes(n, total, p.tile_rows, p.band)
    sb = need if scratch_bytes_ is None else int(scratch_bytes_)
    scratch = torch.empty(max(need, 16) // 4 + 4, dtype=torch.int32, device=dev)
    rows = torch.zeros((max(n, 1), 4), dtype=torch.int64, device=dev)
    lo = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    hi = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_sdtw_band_dev(n, queries.data_ptr() if total else None, first.data_ptr(), qlen.data_ptr(), total,
                                         ref_tensor.data_ptr() if ref_tensor.numel() else None, int(ref_tensor.numel()), anchor.data_ptr(), status.data_ptr(),
                                         C.byref(p), scratch.data_ptr(), sb, rows.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_sdtw_band_dev")
    for t in (queries, first, ref_tensor, qlen, anchor, status, scratch):
        t.record_stream(torch.cuda.current_stream(dev))
    return rows[:n], lo[:total], hi[:total]


def _refine_params(refine):
    """None: no refinement; True: the defaults; else an s5gpu_refine_params_t (refine.RefineParams(...))"""
    return None if refine is None or refine is False else RefineParams() if refine is True else refine


def fit_long_dev(queries, first, qlen, ref_tensor, lo, hi, status=None, params=None, want_queries=True):
    """k_path_fit_long, k_fit_long_solve and k_requant_long behind the plan and check passes of the whole-read pileup -> (fit, queries',
    status'): fit an [n, 8] int64 tensor whose rows are FIT records (fit.cpu().numpy().view(FIT)), queries' [total_rows] int16 (q' at the rows
    of the reads whose status' is 0, zeros elsewhere; None without want_queries), status' [n] int32.  Asynchronous, on the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 1 or ref_tensor.dim() != 1:
        raise ValueError("fit_long_dev: queries [total_rows] and ref_tensor [R] are int16 tensors")
    n, total, dev = int(first.numel()) - 1, int(queries.numel()), queries.device
    p = params if params is not None else RefineParams()
    queries, first, ref_tensor = queries.contiguous(), first.contiguous(), ref_tensor.contiguous()
    qlen, lo, hi = qlen.to(torch.int32).contiguous(), lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev) if status is None else status.to(torch.int32).contiguous()
    wb = int(_lib.lib().s5gpu_path_fit_long_work_bytes(n, total))
    work = torch.empty(max(wb, 16) // 8 + 2, dtype=torch.int64, device=dev)
    fit = torch.zeros((max(n, 1), 8), dtype=torch.int64, device=dev)
    q1 = torch.zeros(max(total, 1), dtype=torch.int16, device=dev) if want_queries else None
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_path_fit_long_dev(n, queries.data_ptr() if total else None, first.data_ptr(), qlen.data_ptr(), total,
                                             ref_tensor.data_ptr() if ref_tensor.numel() else None, int(ref_tensor.numel()), lo.data_ptr() if total else None,
                                             hi.data_ptr() if total else None, status.data_ptr(), C.byref(p), work.data_ptr(), wb, fit.data_ptr(),
                                             q1.data_ptr() if want_queries else None, st.data_ptr(),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_path_fit_long_dev")
    for t in (queries, first, ref_tensor, qlen, lo, hi, status, work):
        t.record_stream(torch.cuda.current_stream(dev))
    return fit[:n], (q1[:total] if want_queries else None), st[:n]


def refine_long_dev(queries, first, qlen, ref_tensor, rows, lo, hi, band_params=None, params=None, scratch_bytes_=None):
    """s5gpu_extend_refine_dev on what band_dev left on the device -> RefinedLong(queries, rows, lo, hi, fit, rounds), all on the device:
    queries [total_rows] int16, rows [n, 4] int64 (EXT_ROW records; a read's status is its row's), lo and hi [total_rows] int32, fit
    [n, 8] int64 (FIT records), rounds [n] int32.  band_params: the BandParams of the band call (tile_rows and band count).
    scratch_bytes_ (for tests): the size the call is told instead of what it needs.  Asynchronous, on the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 1 or ref_tensor.dim() != 1:
        raise ValueError("refine_long_dev: queries [total_rows] and ref_tensor [R] are int16 tensors")
    n, total, dev = int(first.numel()) - 1, int(queries.numel()), queries.device
    bp = band_params if band_params is not None else BandParams()
    p = params if params is not None else RefineParams()
    queries, first, ref_tensor, rows = queries.contiguous(), first.contiguous(), ref_tensor.contiguous(), rows.contiguous()
    qlen, lo, hi = qlen.to(torch.int32).contiguous(), lo.to(torch.int32).contiguous(), hi.to(torch.int32).contiguous()
    need = scratch_bytes(n, total, bp.tile_rows, bp.band)
    sb = need if scratch_bytes_ is None else int(scratch_bytes_)
    scratch = torch.empty(max(need, 16) // 4 + 4, dtype=torch.int32, device=dev)
    wb = int(_lib.lib().s5gpu_extend_refine_work_bytes(n, total))
    work = torch.empty(max(wb, 16) // 8 + 2, dtype=torch.int64, device=dev)
    q1 = torch.zeros(max(total, 1), dtype=torch.int16, device=dev)
    rows1 = torch.zeros((max(n, 1), 4), dtype=torch.int64, device=dev)
    lo1 = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    hi1 = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    fit = torch.zeros((max(n, 1), 8), dtype=torch.int64, device=dev)
    rounds = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_extend_refine_dev(n, queries.data_ptr() if total else None, first.data_ptr(), qlen.data_ptr(), total,
                                             ref_tensor.data_ptr() if ref_tensor.numel() else None, int(ref_tensor.numel()), rows.data_ptr(),
                                             lo.data_ptr() if total else None, hi.data_ptr() if total else None, C.byref(bp), C.byref(p), scratch.data_ptr(), sb,
                                             work.data_ptr(), wb, q1.data_ptr(), rows1.data_ptr(), lo1.data_ptr(), hi1.data_ptr(), fit.data_ptr(),
                                             rounds.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_extend_refine_dev")
    for t in (queries, first, ref_tensor, rows, qlen, lo, hi, scratch, work):
        t.record_stream(torch.cuda.current_stream(dev))
    return RefinedLong(q1[:total], rows1[:n], lo1[:total], hi1[:total], fit[:n], rounds[:n])


def extend_dev(dec, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=EMAX, tile_rows=TILE_ROWS, band=BAND, host=True,
               events=None, refine=None):
    """events, the prefix queries, sDTW with the start, the long queries and the banded alignment from `start`, on what
    press.decode_to_device left on the device -> (MAP_ROW array of the prefix mapping, Extended(rows, first, queries, qlen, lo, hi)).
    host=True: numpy arrays (rows an EXT_ROW array, first uint64); False: the device tensors, and the prefix rows as an [n, 4] int32 tensor.
    ref: the quantised reference, an int16 numpy array or a device tensor.  The prefix query is rows [skip, skip + qmax) of a read, at least
    qmin of them; the long query rows [skip, skip + emax), with the same skip, scale and clip.  events: the (rows, first) that
    events.events_dev(dec, event_params, "raw") returned, for a caller that has them already.  refine (None; True: the defaults; or
    refine.RefineParams(...)): the rounds of refine_long_dev follow, and an ExtendedRefined comes back in Extended's place: rows, queries, lo
    and hi are the refined ones, rows_first the rows of the first alignment, fit a FIT array and rounds [n] (§4.24)."""
    import torch

    ev, first = _events.events_dev(dec, event_params, "raw") if events is None else events
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()          # s5gpu_rec_fields_t.status
    q, ql, st = _map.queries_dev(ev, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    out = _map.sdtw_dev(q, ql, r, True)
    p = BandParams(skip, qmin, emax, tile_rows, band, clip, scale)
    lq, lql, lst = queries_long_dev(ev, first, st, p)
    rows, lo, hi = band_dev(lq, first, lql, r, out[:, 2], lst, p)
    rp = _refine_params(refine)
    if rp is not None:
        x = refine_long_dev(lq, first, lql, r, rows, lo, hi, p, rp)
        if not host:
            return out, ExtendedRefined(x.rows, first, x.queries, lql, x.lo, x.hi, rows, x.fit, x.rounds)
        return out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), ExtendedRefined(
            x.rows.cpu().numpy().view(EXT_ROW).reshape(-1).copy(), first.cpu().numpy().astype(np.uint64), x.queries.cpu().numpy(), lql.cpu().numpy(),
            x.lo.cpu().numpy(), x.hi.cpu().numpy(), rows.cpu().numpy().view(EXT_ROW).reshape(-1).copy(), x.fit.cpu().numpy().view(FIT).reshape(-1).copy(),
            x.rounds.cpu().numpy())
    if not host:
        return out, Extended(rows, first, lq, lql, lo, hi)
    return out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), Extended(rows.cpu().numpy().view(EXT_ROW).reshape(-1).copy(),
                                                                        first.cpu().numpy().astype(np.uint64), lq.cpu().numpy(), lql.cpu().numpy(),
                                                                        lo.cpu().numpy(), hi.cpu().numpy())


def read_extend(records, ref, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
                emax=EMAX, tile_rows=TILE_ROWS, band=BAND, scratch_max=0, raise_on_error=True, refine=None):
    """A batch of records (bytes without the u64 prefix) against the quantised reference `ref` (int16) through s5gpu_extend_batch ->
    (map_rows, rows, first, lo, hi, events, status): a MAP_ROW array (the prefix mapping), an EXT_ROW array, the [n + 1] uint64 prefix of
    rows["qlen"], and ragged along it lo, hi (int32) and the query's event rows (EVENT); status [n] int32.  scratch_max: the bytes of scratch
    a group of reads may use (0: 1 GiB).  A corrupt record raises; with raise_on_error=False it has its status and empty outputs.
    refine (as in extend_dev): through s5gpu_extend_refine_batch -> (map_rows, rows, first, lo, hi, events, status, rows_first, queries, fit,
    rounds): rows, first, lo and hi are the refined ones, queries the refined long queries laid out as lo."""
    L = _lib.lib()
    rp = _refine_params(refine)
    n = len(records)
    ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
    bp = BandParams(skip, qmin, emax, tile_rows, band, clip, scale)
    r = np.ascontiguousarray(ref, dtype=np.int16)
    vp = C.c_void_p
    rb = [bytes(x) for x in records]
    rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
    map_rows, rows = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=EXT_ROW)
    first, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    cap = max(sum(len(x) for x in rb) // 16, 64)
    for _ in range(2):
        lo, hi, ev = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=EVENT)
        if rp is not None:
            rows_first, q1, fit, rounds = np.zeros(n, dtype=EXT_ROW), np.zeros(cap, dtype=np.int16), np.zeros(n, dtype=FIT), np.zeros(n, dtype=np.uint32)
            rc = L.s5gpu_extend_refine_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), C.byref(bp), C.byref(rp), int(scratch_max),
                                             r.ctypes.data_as(vp), len(r), map_rows.ctypes.data_as(vp), rows_first.ctypes.data_as(vp), rows.ctypes.data_as(vp),
                                             first.ctypes.data_as(vp), lo.ctypes.data_as(vp), hi.ctypes.data_as(vp), ev.ctypes.data_as(vp), q1.ctypes.data_as(vp),
                                             cap, fit.ctypes.data_as(vp), rounds.ctypes.data_as(vp), status.ctypes.data_as(vp))
            if rc != -3 or int(first[0]) <= cap:
                break
            cap = int(first[0])
            continue
        rc = L.s5gpu_extend_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), C.byref(bp), int(scratch_max), r.ctypes.data_as(vp), len(r),
                                  map_rows.ctypes.data_as(vp), rows.ctypes.data_as(vp), first.ctypes.data_as(vp), lo.ctypes.data_as(vp), hi.ctypes.data_as(vp),
                                  ev.ctypes.data_as(vp), cap, status.ctypes.data_as(vp))
        if rc != -3 or int(first[0]) <= cap:
            break
        cap = int(first[0])                                                # S5GPU_ERR_NOMEM: first[0] = the rows that suffice
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_extend_batch" if rp is None else "s5gpu_extend_refine_batch")
    t = int(first[n])
    if rp is not None:
        return map_rows, rows, first, lo[:t].copy(), hi[:t].copy(), ev[:t].copy(), status, rows_first, q1[:t].copy(), fit, rounds
    return map_rows, rows, first, lo[:t].copy(), hi[:t].copy(), ev[:t].copy(), status


def file_extend(path, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, emax=None, tile_rows=None, band=None, raise_on_corrupt=True,
                refine=False, iters=None, slope=None):
    """(ids, lines) of a .blow5 file against the levels of ref_path (one number per line), the reads in file order: ids a list of bytes,
    lines an EXTEND_LINE array.  Runs the s5extend tool (examples/s5extend.c), `batch` records per device call.  A corrupt record raises;
    with raise_on_corrupt=False it is left out.  refine=True: `s5extend --refine` (iters: --iters N; slope: --slope LO,HI as a pair), and
    lines is an EXTEND_REFINE_LINE array."""
    if not os.path.exists(S5EXTEND):
        _build.build()
    cmd = [S5EXTEND, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin))]
    cmd += (["--rna"] if rna else []) + (["--max-events", str(int(emax))] if emax is not None else [])
    cmd += (["--tile", str(int(tile_rows))] if tile_rows is not None else []) + (["--band", str(int(band))] if band is not None else [])
    if refine:
        cmd += ["--refine"] + (["--iters", str(int(iters))] if iters is not None else [])
        cmd += ["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []
    p = subprocess.run(cmd + [os.fspath(ref_path), os.fspath(path)], capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5extend %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    ids, lines = [], []

    def num(x, f=int, none=-1):
        return none if x == b"*" else f(x)
    for ln in p.stdout.split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            ids.append(f[0])
            line = (num(f[1]), num(f[2]), num(f[3], float, np.nan), num(f[4]), num(f[5]), num(f[6]), num(f[7]))
            if refine:
                line += (num(f[8], float, np.nan), num(f[9], float, np.nan), num(f[10]), num(f[11]), num(f[12]), num(f[13]), f[14])
            lines.append(line)
    return ids, np.array(lines, dtype=EXTEND_REFINE_LINE if refine else EXTEND_LINE).reshape(-1)
