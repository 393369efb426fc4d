"""sites: which reads differ at a position — per-read levels at chosen reference columns, each held against a control histogram of contrast
(include/slow5gpu.h "sites", docs/codecs.md §4.25).

The matrix is site-major: cells[t, k] (SITE_CELL, 16 bytes) sums the rows i of read k with lo[i] <= sites[t] <= hi[i]: their count, the sum
of their quantised levels and the first such row; {0, 0, 0xFFFFFFFF} where the read is not used or does not cross the site.  A score row
(SITE_SCORE, 16 bytes) holds the entry's level (the mean rounded half up) and, with b its bin, how many of the control's cells at that column
lie in bins <= b (below), >= b (above) and in all (n).  tail() = min(1, 2 min(below, above) / n) is an empirical tail share, not a calibrated
probability, and a read that was itself added to the control counts among its own control.

  check_sites    : a site list as a strictly increasing uint32 array below R, or ValueError
  cells_long_dev : queries, first, qlen, lo, hi and status as extend.band_dev left them -> (cells [M, n, 2] int64 tensor, verdict [n])
  cells_dev      : the same for a fixed-pitch batch ([n, qpitch] arrays as align.path_dev left them)
  score_dev      : a cells tensor and a histogram tensor of contrast -> a scores tensor [M, n, 2] int64
  cells_to_host, scores_to_host : the tensors as SITE_CELL / SITE_SCORE arrays [M, n]
  sites_whole_dev: a DecodedDev (and a control DecodedDev or histogram) -> extend, the cells and the scores; nothing else comes to the host
  Sites          : records -> a per-file handle (s5gpu_sites_add_control / _set_control / _add_batch); close() -> the control histogram
  file_sites     : a .blow5 file, a reference file and a site list -> a SITES_LINE array through the s5sites tool
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from . import _lib
from . import build as _build
from . import contrast as _contrast
from . import events as _events
from . import extend as _extend
from . import map as _map
from . import pileup as _pileup
from ._lib import REC_ZLIB, SIG_SVB_ZD, check
from .contrast import Q0, SHIFT
from .events import DNA
from .map import CLIP, QMAX, QMIN, SCALE, SKIP

SITE_CELL, SITE_SCORE = _lib.SiteCell, _lib.SiteScore
# a line of the tool; below, above and n are -1 and tail is nan without a control
SITES_LINE = np.dtype([("read_id", "U64"), ("ref_pos", "<i8"), ("cells", "<u4"), ("level", "<i4"), ("first_event", "<i8"), ("below", "<i8"), ("above", "<i8"),
                       ("n", "<i8"), ("tail", "<f8")])
MMAX, ENTRIES_MAX, ROW_NONE = 1 << 16, 1 << 27, 0xFFFFFFFF
NO_CELL, EMPTY, COLUMN, HEAD = 1, 2, 64, 128                                # SITE_SCORE.flags
ERR_DATA = -5
S5SITES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5sites")


def check_sites(sites, R):
    """the list as a contiguous uint32 array: 1 .. 65536 columns, strictly increasing, each below R; ValueError otherwise"""
    s = np.asarray(sites)
    if s.ndim != 1 or not 1 <= len(s) <= MMAX or s.dtype.kind not in "iu":
        raise ValueError("sites: 1 .. 65536 integer columns")
    s = s.astype(np.int64)
    if (s < 0).any() or (s >= int(R)).any():
        raise ValueError("sites: a column outside 0 .. R - 1 = %d" % (int(R) - 1))
    if (np.diff(s) <= 0).any():
        raise ValueError("sites: the list is not strictly increasing")
    return np.ascontiguousarray(s, dtype=np.uint32)


def _stream(dev):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _sites_dev(sites, R, dev):
    import torch

    return torch.from_numpy(check_sites(sites, R).view(np.int32)).to(dev)


def cells_long_dev(queries, first, qlen, lo, hi, status, sites, R):
    """The ragged call: queries [total_rows] int16, first [n + 1] int64, qlen [n] int32, lo and hi [total_rows] int32 and status [n] int32 on
    one device; sites a list of columns (validated here).  Asynchronous, on the current stream.  Returns (cells, verdict): an [M, n, 2] int64
    tensor, a SITE_CELL each (cells_to_host), and an [n] int32 tensor: 0 used, 1 skipped, 2 bad."""
    import torch

    if queries.dtype != torch.int16 or queries.dim() != 1:
        raise ValueError("cells_long_dev: queries is a [total_rows] int16 tensor")
    n, total = int(first.numel()) - 1, int(queries.numel())
    if first.dtype != torch.int64 or n < 0 or int(qlen.numel()) != n or int(status.numel()) != n:
        raise ValueError("cells_long_dev: first is an [n + 1] int64 tensor, qlen and status have n entries")
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (total,) or tuple(hi.shape) != (total,):
        raise ValueError("cells_long_dev: lo and hi are [total_rows] int32 tensors")
    dev = queries.device
    s = _sites_dev(sites, R, dev)
    M = int(s.numel())
    if M * n > ENTRIES_MAX:
        raise ValueError("cells_long_dev: %d sites of %d reads (at most 2^27 entries)" % (M, n))
    queries, first, lo, hi = queries.contiguous(), first.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    need = _pileup.work_bytes_long(n, total)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    flat = torch.empty(max(2 * M * n, 2), dtype=torch.int64, device=dev)   # (an entry's room even for n = 0: the call wants a pointer)
    cells = flat[:2 * M * n].view(M, n, 2)
    verdict = torch.empty(n, dtype=torch.int32, device=dev)

    def ptr(t):
        return t.data_ptr() if t.numel() else None
    check(_lib.lib().s5gpu_site_cells_long_dev(n, ptr(queries), first.data_ptr(), ptr(qlen), total, int(R), ptr(lo), ptr(hi), ptr(status), s.data_ptr(), M,
                                               work.data_ptr(), need, flat.data_ptr(), ptr(verdict), _stream(dev)), "s5gpu_site_cells_long_dev")
    for t in (queries, first, lo, hi, qlen, status, work, s):
        t.record_stream(torch.cuda.current_stream(dev))
    return cells, verdict


def cells_dev(queries, qlen, lo, hi, status, sites, R):
    """A fixed-pitch batch (queries, lo and hi [n, qpitch], as align.path_dev left them): the ragged layout with first[k] = k qpitch, a read's
    rows its qlen clamped to the pitch."""
    import torch

    if queries.dim() != 2 or tuple(lo.shape) != tuple(queries.shape) or tuple(hi.shape) != tuple(queries.shape):
        raise ValueError("cells_dev: queries, lo and hi are [n, qpitch] tensors")
    n, pitch = int(queries.shape[0]), int(queries.shape[1])
    first = torch.arange(n + 1, dtype=torch.int64, device=queries.device) * pitch
    ql = qlen.to(torch.int32).clamp(max=pitch)
    return cells_long_dev(queries.contiguous().view(-1), first, ql, lo.contiguous().view(-1), hi.contiguous().view(-1), status, sites, R)


def score_dev(cells, sites, hist):
    """k_site_score: the cells tensor of cells_long_dev for the same site list against a histogram tensor of contrast -> an [M, n, 2] int64
    tensor, a SITE_SCORE each (scores_to_host).  Asynchronous, on the current stream."""
    import torch

    R = _contrast._columns(hist)
    if cells.dtype != torch.int64 or cells.dim() != 3 or int(cells.shape[2]) != 2 or not cells.is_contiguous():
        raise ValueError("score_dev: cells is the [M, n, 2] int64 tensor of cells_long_dev")
    dev = cells.device
    s = _sites_dev(sites, R, dev)
    M, n = int(cells.shape[0]), int(cells.shape[1])
    if int(s.numel()) != M:
        raise ValueError("score_dev: %d sites, a matrix of %d" % (int(s.numel()), M))
    out = torch.empty((M, n, 2), dtype=torch.int64, device=dev)
    if n:
        check(_lib.lib().s5gpu_site_score_dev(cells.data_ptr(), n, s.data_ptr(), M, hist.data_ptr(), R, out.data_ptr(), _stream(dev)), "s5gpu_site_score_dev")
    s.record_stream(torch.cuda.current_stream(dev))
    return out


def cells_to_host(cells):
    """the tensor of cells_long_dev -> a SITE_CELL array [M, n]"""
    return cells.cpu().numpy().view(SITE_CELL).reshape(cells.shape[0], cells.shape[1]).copy()


def scores_to_host(scores):
    """the tensor of score_dev -> a SITE_SCORE array [M, n]"""
    return scores.cpu().numpy().view(SITE_SCORE).reshape(scores.shape[0], scores.shape[1]).copy()


def tail(scores):
    """min(1, 2 min(below, above) / n) of a SITE_SCORE array, nan where there is no cell or no control: an empirical tail share"""
    s = np.asarray(scores)
    n = s["n"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.minimum(1.0, 2.0 * np.minimum(s["below"], s["above"]).astype(np.float64) / n)
    return np.where((s["flags"] & (NO_CELL | EMPTY | HEAD)) != 0, np.nan, t)


def sites_whole_dev(dec, ref, sites, control=None, q0=Q0, shift=SHIFT, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
                    emax=_extend.EMAX, tile_rows=_extend.TILE_ROWS, band=_extend.BAND, refine=None):
    """extend.extend_dev(host=False) on a decoded batch and its ragged paths into the site matrix.  control: None, a histogram tensor of
    contrast, or a DecodedDev whose reads are run through the same chain into a histogram of their own.  Returns (cells, verdict, scores,
    hist, x): scores and hist None without a control, x the ExtendDev of the batch (rows, first, qlen, lo, hi), all on the device.  refine as
    in extend.extend_dev: both batches are fed with the refined queries, paths and statuses."""
    import torch

    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec.dev)
    R = int(r.numel())

    def chain(d):
        ev, first = _events.events_dev(d, event_params, "raw")
        _, x = _extend.extend_dev(d, r, event_params, skip, qmax, qmin, scale, clip, emax, tile_rows, band, host=False, events=(ev, first), refine=refine)
        return x, (x.rows[:, 3] >> 32).to(torch.int32)                     # EXT_ROW.status
    hist = control
    if control is not None and not isinstance(control, torch.Tensor):
        xc, st = chain(control)
        hist = _contrast.hist_accum_long_dev(xc.queries, xc.first, xc.qlen, xc.lo, xc.hi, st, _contrast.new_hist(R, q0, shift, dec.dev))
    x, st = chain(dec)
    cells, verdict = cells_long_dev(x.queries, x.first, x.qlen, x.lo, x.hi, st, sites, R)
    scores = score_dev(cells, sites, hist) if hist is not None else None
    return cells, verdict, scores, hist, x


class Sites:
    """The site matrix of a file on the first device in use: add_control(records) or set_control((head, counts)) for the control, add(records)
    per batch -> its cells and scores, close() -> the control histogram (head, counts) and the end of the handle.  ref: the quantised
    reference (int16).  Also a context manager: leaving it abandons a handle that was not closed."""

    def __init__(self, ref, sites, q0=Q0, shift=SHIFT, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=_extend.EMAX,
                 tile_rows=_extend.TILE_ROWS, band=_extend.BAND, scratch_max=0, refine=None):
        r = np.ascontiguousarray(ref, dtype=np.int16)
        self.sites = check_sites(sites, len(r))
        ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
        bp = _extend.BandParams(skip, qmin, emax, tile_rows, band, clip, scale)
        self.R, self.M = len(r), len(self.sites)
        vp = C.c_void_p
        self._h = _lib.lib().s5gpu_sites_open(C.byref(ep), C.byref(mp), C.byref(bp), int(scratch_max), r.ctypes.data_as(vp), len(r), self.sites.ctypes.data_as(vp),
                                              self.M, int(q0), int(shift))
        if not self._h:
            raise _lib.S5GpuError("s5gpu_sites_open failed: %s" % _lib.lib().s5gpu_last_error().decode(errors="replace"))
        rp = _extend._refine_params(refine)
        if rp is not None:
            rc = _lib.lib().s5gpu_sites_set_refine(self._h, C.byref(rp))
            if rc != 0:
                self.abandon()
                check(rc, "s5gpu_sites_set_refine")

    def _records(self, records):
        if self._h is None:
            raise _lib.S5GpuError("sites handle: already closed")
        n = len(records)
        rb = [bytes(x) for x in records]
        rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
        rec_p = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in rbuf])
        rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
        return n, rbuf, rec_p, rl

    def add_control(self, records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        """Adds a batch of records (bytes without the u64 prefix) to the control histogram -> (rc, status).  A corrupt record raises after the
        rest of the batch has been added; with raise_on_error=False rc is -5 and the record shows in its status."""
        n, _keep, rec_p, rl = self._records(records)
        status = np.zeros(n, dtype=np.int32)
        rc = _lib.lib().s5gpu_sites_add_control(self._h, n, rec_p, rl, rec_method, sig_method, status.ctypes.data_as(C.c_void_p))
        if rc != 0 and (raise_on_error or rc != ERR_DATA):
            check(rc, "s5gpu_sites_add_control")
        return rc, status

    def set_control(self, hist):
        """the control replaced by a histogram made elsewhere: (head, counts) as contrast.hist_to_host gives it, or its bytes"""
        if self._h is None:
            raise _lib.S5GpuError("sites handle: already closed")
        raw = bytes(hist) if isinstance(hist, (bytes, bytearray)) else np.array([hist[0]]).tobytes() + np.ascontiguousarray(hist[1], dtype="<u4").tobytes()
        if len(raw) != _contrast.hist_bytes(self.R):
            raise ValueError("set_control: not a histogram of %d columns" % self.R)
        buf = np.frombuffer(raw, dtype=np.uint8).copy()
        check(_lib.lib().s5gpu_sites_set_control(self._h, buf.ctypes.data_as(C.c_void_p)), "s5gpu_sites_set_control")

    def add(self, records, scores=True, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        """A batch of records -> (rc, EXT_ROW array, cells [M, n], scores [M, n] or None, status).  The control is not changed.  A corrupt
        record raises; with raise_on_error=False rc is -5, its entries are empty and it shows in its status.  The handle stays usable."""
        n, _keep, rec_p, rl = self._records(records)
        if self.M * n > ENTRIES_MAX:
            raise ValueError("Sites.add: %d sites of %d records (at most 2^27 entries)" % (self.M, n))
        vp = C.c_void_p
        rows, status = np.zeros(n, dtype=_extend.EXT_ROW), np.zeros(n, dtype=np.int32)
        cells = np.zeros((self.M, n), dtype=SITE_CELL)
        sc = np.zeros((self.M, n), dtype=SITE_SCORE) if scores else None
        rc = _lib.lib().s5gpu_sites_add_batch(self._h, n, rec_p, rl, rec_method, sig_method, rows.ctypes.data_as(vp), cells.ctypes.data_as(vp),
                                              sc.ctypes.data_as(vp) if scores else None, status.ctypes.data_as(vp))
        if rc != 0 and (raise_on_error or rc != ERR_DATA):
            check(rc, "s5gpu_sites_add_batch")
        return rc, rows, cells, sc, status

    def close(self):
        if self._h is None:
            raise _lib.S5GpuError("sites handle: already closed")
        raw = np.zeros(_contrast.hist_bytes(self.R), dtype=np.uint8)
        h, self._h = self._h, None
        check(_lib.lib().s5gpu_sites_close(h, raw.ctypes.data_as(C.c_void_p)), "s5gpu_sites_close")
        return _contrast.hist_from_bytes(raw.tobytes())

    def abandon(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().s5gpu_sites_close(h, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.abandon()
        return False


def file_sites(path, ref_path, sites, control=None, refine=None, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, q0=Q0, shift=SHIFT, emax=None,
               tile_rows=None, band=None, raise_on_corrupt=True, iters=None, slope=None):
    """The reads of a .blow5 file at the columns `sites` of the levels of ref_path (one number per line) as a SITES_LINE array, a row per read
    and site the read crosses; control: a second .blow5 file, streamed first into the control histogram (without one below, above and n are
    -1 and tail is nan).  Runs the s5sites tool (examples/s5sites.c), `batch` records per device call.  A corrupt record raises; with
    raise_on_corrupt=False it is left out.  refine: None or False for no rounds, True for --refine, with iters and slope as in
    extend.file_extend."""
    s = np.asarray(sites)
    if s.ndim != 1 or not 1 <= len(s) <= MMAX or s.dtype.kind not in "iu" or (s.astype(np.int64) < 0).any() or (np.diff(s.astype(np.int64)) <= 0).any():
        raise ValueError("file_sites: 1 .. 65536 columns, strictly increasing")
    if not os.path.exists(S5SITES):
        _build.build()
    with tempfile.NamedTemporaryFile("w", suffix=".sites", delete=False) as fh:
        fh.write("".join("%d\n" % int(v) for v in s))
        sites_path = fh.name
    try:
        cmd = [S5SITES, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin)), "--q0", str(int(q0)),
               "--shift", str(int(shift))]
        cmd += (["--rna"] if rna else []) + (["--max-events", str(int(emax))] if emax is not None else [])
        cmd += (["--tile", str(int(tile_rows))] if tile_rows is not None else []) + (["--band", str(int(band))] if band is not None else [])
        if refine:
            cmd += ["--refine"] + (["--iters", str(int(iters))] if iters is not None else [])
            cmd += ["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []
        cmd += (["--control", os.fspath(control)] if control is not None else []) + ["--sites", sites_path, os.fspath(ref_path), os.fspath(path)]
        p = subprocess.run(cmd, capture_output=True)
    finally:
        os.unlink(sites_path)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5sites %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    lines = []
    for ln in p.stdout.split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            ctl = f[5] != b"."
            lines.append((f[0].decode(), int(f[1]), int(f[2]), int(f[3]), int(f[4])) + ((int(f[5]), int(f[6]), int(f[7]), float(f[8])) if ctl else (-1, -1, -1, np.nan)))
    return np.array(lines, dtype=SITES_LINE).reshape(-1)
