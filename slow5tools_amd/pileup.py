"""pileup: what the reads say about each reference position — the transpose of align (align.py), accumulated on the device
(include/slow5gpu.h "pileup", docs/codecs.md §4.18).

The accumulator is a totals row (PILE_TOTAL, 64 bytes) and R columns (PILE_COL, 48 bytes each) that stay on the device while the batches
stream through.  A read is used iff its status is 0, it has a query and its lo / hi form a valid monotone path; column j then counts its
cells (i, j), lo[i] <= j <= hi[i].  Every member is an integer sum, minimum or maximum: the table does not depend on the order of reads,
batches or streams.

  new_acc     : an empty accumulator of R columns as a device tensor
  accum_dev   : k_pileup on queries, qlen, a reference, lo, hi and status as align.path_dev left them, into an accumulator tensor
  to_host     : an accumulator tensor -> (total, cols) numpy records
  pileup_dev  : a DecodedDev -> events, queries, sDTW, paths, then accum_dev
  Pileup      : records -> a per-file handle (s5gpu_pileup_add_batch); close() makes the one download
  file_pileup : a .blow5 file and a reference file -> a PILE_LINE array through the s5pileup tool

Whole reads (§4.22): the same table from all of a read's events, over the ragged paths of extend (extend.py).
  work_bytes_long  : the bytes of the work area of a ragged call
  accum_long_dev   : queries, first, qlen, lo, hi and status as extend.band_dev left them, into an accumulator tensor
  pileup_whole_dev : a DecodedDev -> extend.extend_dev(host=False), then accum_long_dev
  PileupWhole      : records -> a per-file handle (s5gpu_pileup_add_batch_whole)
  file_pileup(whole=True) : s5pileup --whole

Folded (§4.26, model.py): Pileup.close_folded and PileupWhole.close_folded fold the table onto classes on the device before the download.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import align as _align
from . import build as _build
from . import events as _events
from . import extend as _extend
from . import map as _map
from ._lib import REC_ZLIB, SIG_SVB_ZD, check
from .events import DNA, RNA  # noqa: F401  (RNA: for callers)
from .map import CLIP, MAP_ROW, QMAX, QMIN, SCALE, SKIP

PILE_COL, PILE_TOTAL = _lib.PileCol, _lib.PileTotal
# a line of the tool
PILE_LINE = np.dtype([("ref_pos", "<i8"), ("ref_level", "<i4"), ("depth", "<u4"), ("events", "<u4"), ("samples", "<u8"), ("mean", "<f8"), ("stdv", "<f8"),
                      ("min", "<i4"), ("max", "<i4"), ("mean_cost", "<f8")])
RMAX = 1 << 26
ERR_DATA = -5
S5PILEUP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5pileup")


def acc_bytes(R):
    """the bytes of an accumulator of R columns (0: an R the calls refuse)"""
    return int(_lib.lib().s5gpu_pileup_bytes(int(R)))


def new_acc(R, device="cuda:0"):
    """an empty accumulator of R columns as a uint8 tensor on the device (s5gpu_pileup_reset_dev)"""
    import torch

    nb = acc_bytes(R)
    if nb == 0:
        raise ValueError("new_acc: R %d (1 .. 2^26)" % R)
    dev = torch.device(device)
    t = torch.zeros(nb, dtype=torch.uint8, device=dev)
    check(_lib.lib().s5gpu_pileup_reset_dev(t.data_ptr(), int(R), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_pileup_reset_dev")
    return t


def accum_dev(queries, qlen, ref_tensor, lo, hi, status, acc, events=None):
    """k_pileup: queries [n, qpitch] int16, qlen [n] int32, ref_tensor [R] int16, lo and hi [n, qpitch] int32, status [n] int32 and, when
    given, events [n, qpitch, 4] int32 (the query's event rows; only their lengths are read), all on the device of acc, an accumulator of R
    columns.  Asynchronous, on the current stream; the caller keeps the inputs alive until it has run.  Returns acc."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 2 or ref_tensor.dim() != 1:
        raise ValueError("accum_dev: queries [n, qpitch] and ref_tensor [R] are int16 tensors")
    n, pitch, R = int(queries.shape[0]), int(queries.shape[1]), int(ref_tensor.numel())
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (n, pitch) or tuple(hi.shape) != (n, pitch):
        raise ValueError("accum_dev: lo and hi are [n, qpitch] int32 tensors")
    if acc.dtype != torch.uint8 or int(acc.numel()) != acc_bytes(R):
        raise ValueError("accum_dev: acc is not an accumulator of %d columns" % R)
    if events is not None and (events.dtype != torch.int32 or tuple(events.shape) != (n, pitch, 4)):
        raise ValueError("accum_dev: events is an [n, qpitch, 4] int32 tensor")
    queries, ref_tensor, lo, hi = queries.contiguous(), ref_tensor.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    events = events.contiguous() if events is not None else None
    dev = acc.device
    check(_lib.lib().s5gpu_pileup_accum_dev(n, queries.data_ptr(), pitch, qlen.data_ptr(), ref_tensor.data_ptr() if R else None, R, lo.data_ptr(),
                                            hi.data_ptr(), status.data_ptr(), events.data_ptr() if events is not None and n else None, acc.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_pileup_accum_dev")
    for t in (queries, ref_tensor, lo, hi, qlen, status, events):          # (copies made here die with this frame)
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    return acc


def from_bytes(raw):
    """the bytes of an accumulator -> (total, cols): a PILE_TOTAL record and a PILE_COL array of total['R'] rows"""
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    total = b[:64].view(PILE_TOTAL)[0].copy()
    return total, b[64:].view(PILE_COL).copy()


def to_host(acc):
    """an accumulator tensor -> (total, cols)"""
    return from_bytes(acc.cpu().numpy().tobytes())


def pileup_dev(dec, ref, acc, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, wmax=None, scratch_bytes=None):
    """events, queries, sDTW and paths on what press.decode_to_device left on the device, as align.align_dev, then accum_dev into acc; nothing
    comes to the host.  ref: the quantised reference, an int16 numpy array or a device tensor.  Returns (acc, status): status the [n] int32
    device tensor of the reads (0: the read was offered to the table)."""
    import torch

    rows, first = _events.events_dev(dec, event_params, "raw")
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()          # s5gpu_rec_fields_t.status
    q, ql, st = _map.queries_dev(rows, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    out = _map.sdtw_dev(q, ql, r, True)
    lo, hi, pst = _align.path_dev(q, ql, r, out, wmax, scratch_bytes)
    st = torch.where(st != 0, st, pst)
    # the query's event rows as an [n, qmax] matrix, zeros behind qlen (what k_ev_gather leaves in the batch call)
    n, pitch = int(q.shape[0]), int(q.shape[1])
    ev = torch.zeros((n, pitch, 4), dtype=torch.int32, device=dec.dev)
    if n and rows.numel():
        k = torch.arange(pitch, device=dec.dev, dtype=torch.int64)[None, :]
        inside = k < ql.to(torch.int64)[:, None]
        at = (first[:n, None] + int(skip) + k).clamp_(0, int(rows.shape[0]) - 1)
        ev = torch.where(inside[:, :, None], rows[at], ev)
    accum_dev(q, ql, r, lo, hi, st, acc, ev)
    return acc, st


def work_bytes_long(n, total_rows):
    """s5gpu_pileup_long_work_bytes (0: a total_rows the call refuses)"""
    return int(_lib.lib().s5gpu_pileup_long_work_bytes(int(n), int(total_rows)))


def accum_long_dev(queries, first, qlen, ref_tensor, lo, hi, status, acc, events=None, ev_skip=0):
    """The ragged accumulate: queries [total_rows] int16, first [n + 1] int64 (the prefix events.events_dev returns), qlen [n] int32,
    ref_tensor [R] int16, lo and hi [total_rows] int32, status [n] int32 and, when given, events [total_rows, 4] int32 (the reads' event rows;
    the samples of row i of read k are those of row first[k] + ev_skip + i), all on the device of acc, an accumulator of R columns.
    Asynchronous, on the current stream.  Returns acc."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 1 or ref_tensor.dim() != 1:
        raise ValueError("accum_long_dev: queries [total_rows] and ref_tensor [R] are int16 tensors")
    n, total, R = int(first.numel()) - 1, int(queries.numel()), int(ref_tensor.numel())
    if first.dtype != torch.int64 or n < 0 or int(qlen.numel()) != n or int(status.numel()) != n:
        raise ValueError("accum_long_dev: first is an [n + 1] int64 tensor, qlen and status have n entries")
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (total,) or tuple(hi.shape) != (total,):
        raise ValueError("accum_long_dev: lo and hi are [total_rows] int32 tensors")
    if acc.dtype != torch.uint8 or int(acc.numel()) != acc_bytes(R):
        raise ValueError("accum_long_dev: acc is not an accumulator of %d columns" % R)
    if events is not None and (events.dtype != torch.int32 or tuple(events.shape) != (total, 4)):
        raise ValueError("accum_long_dev: events is a [total_rows, 4] int32 tensor")
    queries, first, ref_tensor, lo, hi = queries.contiguous(), first.contiguous(), ref_tensor.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    events = events.contiguous() if events is not None else None
    dev = acc.device
    need = work_bytes_long(n, total)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def ptr(t):
        return t.data_ptr() if t is not None and t.numel() else None
    check(_lib.lib().s5gpu_pileup_accum_long_dev(n, ptr(queries), first.data_ptr(), ptr(qlen), total, ptr(ref_tensor), R, ptr(lo), ptr(hi), ptr(status),
                                                 ptr(events), int(ev_skip), work.data_ptr(), need, acc.data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_pileup_accum_long_dev")
    for t in (queries, first, ref_tensor, lo, hi, qlen, status, events, work):
        if t is not None:
            t.record_stream(torch.cuda.current_stream(dev))
    return acc


def pileup_whole_dev(dec, ref, acc, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=_extend.EMAX,
                     tile_rows=_extend.TILE_ROWS, band=_extend.BAND, refine=None):
    """extend.extend_dev(host=False) on what press.decode_to_device left on the device, then accum_long_dev of all of every read's rows into
    acc; nothing comes to the host.  Returns (acc, status, ext_rows): the [n] int32 statuses of the reads (0: the read was offered to the
    table) and the [n, 4] int64 tensor of EXT_ROW records, both on the device.  refine (as in extend.extend_dev): the table is fed with the
    refined queries, paths and statuses, and ext_rows are the refined rows (§4.24)."""
    import torch

    ev, first = _events.events_dev(dec, event_params, "raw")               # (kept: the samples of a row are its event's length)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    _, x = _extend.extend_dev(dec, r, event_params, skip, qmax, qmin, scale, clip, emax, tile_rows, band, host=False, events=(ev, first), refine=refine)
    st = (x.rows[:, 3] >> 32).to(torch.int32)                              # EXT_ROW.status
    accum_long_dev(x.queries, x.first, x.qlen, r, x.lo, x.hi, st, acc, ev, skip)
    return acc, st, x.rows


class Pileup:
    """One file's table on the first device in use: add(records) per batch, close() -> (total, cols) and the end of the handle.  ref: the
    quantised reference (int16).  Also a context manager: leaving it abandons a handle that was not closed."""

    def __init__(self, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, wmax=None):
        r = np.ascontiguousarray(ref, dtype=np.int16)
        ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
        self.R = len(r)
        self._h = _lib.lib().s5gpu_pileup_open(C.byref(ep), C.byref(mp), 4 * int(qmax) if wmax is None else int(wmax), r.ctypes.data_as(C.c_void_p), len(r))
        if not self._h:
            raise _lib.S5GpuError("s5gpu_pileup_open failed: %s" % _lib.lib().s5gpu_last_error().decode(errors="replace"))

    def add(self, records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        """Adds a batch of records (bytes without the u64 prefix) -> (rc, MAP_ROW array, status).  A corrupt record raises after the rest of
        the batch has been added; with raise_on_error=False rc is -5 and the record shows in its status.  The handle stays usable either way."""
        if self._h is None:
            raise _lib.S5GpuError("pileup handle: already closed")
        n = len(records)
        vp = C.c_void_p
        rb = [bytes(x) for x in records]
        rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
        rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
        rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
        rows, status = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=np.int32)
        rc = _lib.lib().s5gpu_pileup_add_batch(self._h, n, rec_p, rl, rec_method, sig_method, rows.ctypes.data_as(vp), status.ctypes.data_as(vp))
        if rc != 0 and (raise_on_error or rc != ERR_DATA):
            check(rc, "s5gpu_pileup_add_batch")
        return rc, rows, status

    def close(self):
        if self._h is None:
            raise _lib.S5GpuError("pileup handle: already closed")
        out = np.zeros(acc_bytes(self.R), dtype=np.uint8)
        h, self._h = self._h, None
        check(_lib.lib().s5gpu_pileup_close(h, out.ctypes.data_as(C.c_void_p)), "s5gpu_pileup_close")
        return from_bytes(out)

    def close_folded(self, cls, K):
        """close(), with the table folded onto K classes on the device first (s5gpu_pileup_close_folded, §4.26): cls a uint32 class per
        reference column (RefSeq.classes()); -> (total, cols) of K columns.  The handle ends whatever happens."""
        if self._h is None:
            raise _lib.S5GpuError("pileup handle: already closed")
        c = np.ascontiguousarray(cls, dtype=np.uint32)
        h, self._h = self._h, None
        if c.shape != (self.R,) or acc_bytes(K) == 0:
            _lib.lib().s5gpu_pileup_close(h, None)
            raise ValueError("close_folded: cls holds a class per column (%d), K is 1 .. 2^26" % self.R)
        out = np.zeros(acc_bytes(K), dtype=np.uint8)
        check(_lib.lib().s5gpu_pileup_close_folded(h, c.ctypes.data_as(C.c_void_p), int(K), out.ctypes.data_as(C.c_void_p)), "s5gpu_pileup_close_folded")
        return from_bytes(out)

    def abandon(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().s5gpu_pileup_close(h, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.abandon()
        return False


class PileupWhole(Pileup):
    """Pileup for whole reads: add(records) runs extend's chain (s5gpu_pileup_add_batch_whole) and returns (rc, MAP_ROW array of the prefix
    mapping, EXT_ROW array, status).  close, abandon and the context manager are Pileup's."""

    def __init__(self, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=_extend.EMAX, tile_rows=_extend.TILE_ROWS,
                 band=_extend.BAND, scratch_max=0, refine=None):
        r = np.ascontiguousarray(ref, dtype=np.int16)
        ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
        bp = _extend.BandParams(skip, qmin, emax, tile_rows, band, clip, scale)
        self.R = len(r)
        self._h = _lib.lib().s5gpu_pileup_open_whole(C.byref(ep), C.byref(mp), C.byref(bp), int(scratch_max), r.ctypes.data_as(C.c_void_p), len(r))
        if not self._h:
            raise _lib.S5GpuError("s5gpu_pileup_open_whole failed: %s" % _lib.lib().s5gpu_last_error().decode(errors="replace"))
        rp = _extend._refine_params(refine)                                # (§4.24: the rows add() returns are then the refined ones)
        if rp is not None:
            rc = _lib.lib().s5gpu_pileup_set_refine(self._h, C.byref(rp))
            if rc != 0:
                self.abandon()
                check(rc, "s5gpu_pileup_set_refine")

    def add(self, records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        if self._h is None:
            raise _lib.S5GpuError("pileup handle: already closed")
        n = len(records)
        vp = C.c_void_p
        rb = [bytes(x) for x in records]
        rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
        rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
        rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
        map_rows, rows, status = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=_extend.EXT_ROW), np.zeros(n, dtype=np.int32)
        rc = _lib.lib().s5gpu_pileup_add_batch_whole(self._h, n, rec_p, rl, rec_method, sig_method, map_rows.ctypes.data_as(vp), rows.ctypes.data_as(vp),
                                                     status.ctypes.data_as(vp))
        if rc != 0 and (raise_on_error or rc != ERR_DATA):
            check(rc, "s5gpu_pileup_add_batch_whole")
        return rc, map_rows, rows, status


def file_pileup(path, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, wmax=None, min_depth=1, raise_on_corrupt=True, whole=False, emax=None,
                tile_rows=None, band=None, refine=False, iters=None, slope=None):
    """The table of a .blow5 file against the levels of ref_path (one number per line) as a PILE_LINE array, a row per reference position of
    depth >= min_depth.  Runs the s5pileup tool (examples/s5pileup.c), `batch` records per device call.  A corrupt record raises; with
    raise_on_corrupt=False it is left out.  whole=True: the table of whole reads (--whole), with emax, tile_rows and band as in
    extend.file_extend; wmax does not count then.  refine=True (with whole): --refine, with iters and slope as in extend.file_extend."""
    if not os.path.exists(S5PILEUP):
        _build.build()
    cmd = [S5PILEUP, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin)), "--min-depth", str(int(min_depth))]
    cmd += (["--rna"] if rna else []) + (["--max-span", str(int(wmax))] if wmax is not None else [])
    if whole:
        cmd += ["--whole"] + (["--max-events", str(int(emax))] if emax is not None else [])
        cmd += (["--tile", str(int(tile_rows))] if tile_rows is not None else []) + (["--band", str(int(band))] if band is not None else [])
    if refine:
        cmd += ["--refine"] + (["--iters", str(int(iters))] if iters is not None else [])
        cmd += ["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []
    cmd += [os.fspath(ref_path), os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5pileup %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    lines = []
    for ln in p.stdout.split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            lines.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), float(f[5]), float(f[6]), int(f[7]), int(f[8]), float(f[9])))
    return np.array(lines, dtype=PILE_LINE).reshape(-1)
