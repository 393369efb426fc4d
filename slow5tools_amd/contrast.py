"""contrast: where two samples differ — per-reference-position level histograms beside the table of pileup, and a two-sample comparison of
them on the device (include/slow5gpu.h "contrast", docs/codecs.md §4.23).

A histogram is a head (HIST_HEAD, 64 bytes) and R columns of 64 uint32 counts.  The bin of a quantised level q is 0 below q0, else
min((q - q0) >> shift, 63); column j, bin b counts the cells (i, j) of used reads (pileup's rule for whole reads) with bin(q[i]) = b.  A row
of the comparison (CONTRAST_ROW, 40 bytes) holds, all as integers, the numerators of the Kolmogorov-Smirnov statistic and of the overlap of
column j's two histograms: D = ks_num / (n_a n_b), total variation = 1 - ov_num / (n_a n_b).  D is a statistic, not a probability.

  hist_bytes          : the bytes of a histogram of R columns (0: an R the calls refuse)
  new_hist            : an empty histogram as a device tensor
  hist_accum_long_dev : queries, first, qlen, lo, hi and status as extend.band_dev left them, into a histogram tensor
  hist_accum_dev      : the same for a fixed-pitch batch ([n, qpitch] arrays as align.path_dev left them)
  hist_to_host        : a histogram tensor -> (head, counts [R, 64])
  contrast_dev        : two histograms (and the two tables) -> a device tensor of rows; rows_to_host views it as CONTRAST_ROW
  contrast_whole_dev  : two DecodedDev -> extend, both accumulates and the comparison; nothing but the rows need come to the host
  Contrast            : records -> a per-file handle with two sides (s5gpu_contrast_add_batch); close() -> rows and both tables;
                        close_folded(cls, K) -> the same over K classes, such as k-mers (§4.26, model.py)
  file_contrast       : two .blow5 files and a reference file -> a CONTRAST_LINE array through the s5contrast tool
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from . import events as _events
from . import extend as _extend
from . import map as _map
from . import pileup as _pileup
from ._lib import REC_ZLIB, SIG_SVB_ZD, check
from .events import DNA
from .map import CLIP, MAP_ROW, QMAX, QMIN, SCALE, SKIP

HIST_HEAD, CONTRAST_ROW = _lib.PileHistHead, _lib.PileContrast
# a line of the tool
CONTRAST_LINE = np.dtype([("ref_pos", "<i8"), ("ref_level", "<i4"), ("depth_a", "<u4"), ("depth_b", "<u4"), ("events_a", "<u4"), ("events_b", "<u4"),
                          ("mean_a", "<f8"), ("mean_b", "<f8"), ("ks_d", "<f8"), ("ks_level", "<i4"), ("tv", "<f8"), ("med_a", "<i4"), ("med_b", "<i4")])
RMAX, BINS, Q0, SHIFT = 1 << 22, 64, -128, 2
EMPTY_A, EMPTY_B, A_LOWER, BIG, TABLE_A, TABLE_B, HEADS = 1, 2, 4, 8, 16, 32, 128          # CONTRAST_ROW.flags
ERR_DATA = -5
S5CONTRAST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5contrast")


def hist_bytes(R):
    """the bytes of a histogram of R columns (0: an R the calls refuse)"""
    return int(_lib.lib().s5gpu_pile_hist_bytes(int(R)))


def _stream(dev):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def new_hist(R, q0=Q0, shift=SHIFT, device="cuda:0"):
    """an empty histogram of R columns as a uint8 tensor on the device (s5gpu_pile_hist_reset_dev)"""
    import torch

    nb = hist_bytes(R)
    if nb == 0:
        raise ValueError("new_hist: R %d (1 .. 2^22)" % R)
    dev = torch.device(device)
    t = torch.zeros(nb, dtype=torch.uint8, device=dev)
    check(_lib.lib().s5gpu_pile_hist_reset_dev(t.data_ptr(), int(R), int(q0), int(shift), _stream(dev)), "s5gpu_pile_hist_reset_dev")
    return t


def _columns(hist):
    import torch

    if hist.dtype != torch.uint8 or hist.dim() != 1 or int(hist.numel()) < 64 + 256 or (int(hist.numel()) - 64) % 256:
        raise ValueError("not a histogram tensor")
    return (int(hist.numel()) - 64) // 256


def hist_accum_long_dev(queries, first, qlen, lo, hi, status, hist):
    """The ragged accumulate: queries [total_rows] int16, first [n + 1] int64, qlen [n] int32, lo and hi [total_rows] int32 and status [n]
    int32, all on the device of hist.  Asynchronous, on the current stream.  Returns hist."""
    import torch

    R = _columns(hist)
    if queries.dtype != torch.int16 or queries.dim() != 1:
        raise ValueError("hist_accum_long_dev: queries is a [total_rows] int16 tensor")
    n, total = int(first.numel()) - 1, int(queries.numel())
    if first.dtype != torch.int64 or n < 0 or int(qlen.numel()) != n or int(status.numel()) != n:
        raise ValueError("hist_accum_long_dev: first is an [n + 1] int64 tensor, qlen and status have n entries")
    if lo.dtype != torch.int32 or hi.dtype != torch.int32 or tuple(lo.shape) != (total,) or tuple(hi.shape) != (total,):
        raise ValueError("hist_accum_long_dev: lo and hi are [total_rows] int32 tensors")
    queries, first, lo, hi = queries.contiguous(), first.contiguous(), lo.contiguous(), hi.contiguous()
    qlen, status = qlen.to(torch.int32).contiguous(), status.to(torch.int32).contiguous()
    dev = hist.device
    need = _pileup.work_bytes_long(n, total)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def ptr(t):
        return t.data_ptr() if t.numel() else None
    check(_lib.lib().s5gpu_pile_hist_accum_long_dev(n, ptr(queries), first.data_ptr(), ptr(qlen), total, R, ptr(lo), ptr(hi), ptr(status), work.data_ptr(), need,
                                                    hist.data_ptr(), _stream(dev)), "s5gpu_pile_hist_accum_long_dev")
    for t in (queries, first, lo, hi, qlen, status, work):
        t.record_stream(torch.cuda.current_stream(dev))
    return hist


def hist_accum_dev(queries, qlen, lo, hi, status, hist):
    """A fixed-pitch batch (queries, lo and hi [n, qpitch], as align.path_dev left them): the ragged layout with first[k] = k qpitch, a read's
    rows its qlen clamped to the pitch."""
    import torch

    if queries.dim() != 2 or tuple(lo.shape) != tuple(queries.shape) or tuple(hi.shape) != tuple(queries.shape):
        raise ValueError("hist_accum_dev: queries, lo and hi are [n, qpitch] tensors")
    n, pitch = int(queries.shape[0]), int(queries.shape[1])
    first = torch.arange(n + 1, dtype=torch.int64, device=hist.device) * pitch
    ql = qlen.to(torch.int32).clamp(max=pitch)
    return hist_accum_long_dev(queries.contiguous().view(-1), first, ql, lo.contiguous().view(-1), hi.contiguous().view(-1), status, hist)


def hist_from_bytes(raw):
    """the bytes of a histogram -> (head, counts): a HIST_HEAD record and an [R, 64] uint32 array"""
    b = np.frombuffer(bytes(raw), dtype=np.uint8)
    return b[:64].view(HIST_HEAD)[0].copy(), b[64:].view("<u4").reshape(-1, BINS).copy()


def hist_to_host(hist):
    """a histogram tensor -> (head, counts)"""
    return hist_from_bytes(hist.cpu().numpy().tobytes())


def contrast_dev(hist_a, hist_b, acc_a=None, acc_b=None):
    """k_pile_contrast on two histogram tensors of the same R and, when given, the two accumulator tensors of pileup for the same reads ->
    an [R, 5] int64 device tensor, a CONTRAST_ROW each (rows_to_host).  Asynchronous, on the current stream."""
    import torch

    R = _columns(hist_a)
    if _columns(hist_b) != R or (acc_a is None) != (acc_b is None):
        raise ValueError("contrast_dev: two histograms of the same R; both tables or neither")
    for acc in (acc_a, acc_b):
        if acc is not None and (acc.dtype != torch.uint8 or int(acc.numel()) != _pileup.acc_bytes(R)):
            raise ValueError("contrast_dev: acc is not an accumulator of %d columns" % R)
    dev = hist_a.device
    out = torch.zeros((R, 5), dtype=torch.int64, device=dev)
    check(_lib.lib().s5gpu_pile_contrast_dev(hist_a.data_ptr(), hist_b.data_ptr(), acc_a.data_ptr() if acc_a is not None else None,
                                             acc_b.data_ptr() if acc_b is not None else None, R, out.data_ptr(), _stream(dev)), "s5gpu_pile_contrast_dev")
    return out


def rows_to_host(rows):
    """the tensor of contrast_dev -> a CONTRAST_ROW array"""
    return rows.cpu().numpy().view(CONTRAST_ROW).reshape(-1).copy()


def contrast_whole_dev(dec_a, dec_b, ref, q0=Q0, shift=SHIFT, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=_extend.EMAX,
                       tile_rows=_extend.TILE_ROWS, band=_extend.BAND, refine=None):
    """extend.extend_dev(host=False) on two decoded batches, each side's ragged paths into a table and a histogram of its own, then
    contrast_dev.  Returns (rows, (acc_a, acc_b), (hist_a, hist_b)), all on the device.  refine (as in extend.extend_dev): both sides are
    fed with the refined queries, paths and statuses: the bins are then in the reference's units (§4.24)."""
    import torch

    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    r = r.to(dec_a.dev)
    R = int(r.numel())
    accs, hists = [], []
    for dec in (dec_a, dec_b):
        ev, first = _events.events_dev(dec, event_params, "raw")
        _, x = _extend.extend_dev(dec, r, event_params, skip, qmax, qmin, scale, clip, emax, tile_rows, band, host=False, events=(ev, first), refine=refine)
        st = (x.rows[:, 3] >> 32).to(torch.int32)                          # EXT_ROW.status
        accs.append(_pileup.accum_long_dev(x.queries, x.first, x.qlen, r, x.lo, x.hi, st, _pileup.new_acc(R, dec.dev), ev, skip))
        hists.append(hist_accum_long_dev(x.queries, x.first, x.qlen, x.lo, x.hi, st, new_hist(R, q0, shift, dec.dev)))
    return contrast_dev(hists[0], hists[1], accs[0], accs[1]), tuple(accs), tuple(hists)


class Contrast:
    """Two files' tables and histograms on the first device in use: add(side, records) per batch, close() -> (rows, (total_a, cols_a),
    (total_b, cols_b)) and the end of the handle.  ref: the quantised reference (int16).  Also a context manager: leaving it abandons a
    handle that was not closed."""

    def __init__(self, ref, q0=Q0, shift=SHIFT, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, emax=_extend.EMAX,
                 tile_rows=_extend.TILE_ROWS, band=_extend.BAND, scratch_max=0, refine=None):
        r = np.ascontiguousarray(ref, dtype=np.int16)
        ep, mp = _events._params(event_params), _map._params(skip, qmax, qmin, scale, clip, True)
        bp = _extend.BandParams(skip, qmin, emax, tile_rows, band, clip, scale)
        self.R = len(r)
        self._h = _lib.lib().s5gpu_contrast_open(C.byref(ep), C.byref(mp), C.byref(bp), int(scratch_max), r.ctypes.data_as(C.c_void_p), len(r), int(q0), int(shift))
        if not self._h:
            raise _lib.S5GpuError("s5gpu_contrast_open failed: %s" % _lib.lib().s5gpu_last_error().decode(errors="replace"))
        rp = _extend._refine_params(refine)
        if rp is not None:
            rc = _lib.lib().s5gpu_contrast_set_refine(self._h, C.byref(rp))
            if rc != 0:
                self.abandon()
                check(rc, "s5gpu_contrast_set_refine")

    def add(self, side, records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        """Adds a batch of records (bytes without the u64 prefix) to side 0 or 1 -> (rc, MAP_ROW array, EXT_ROW array, status).  A corrupt
        record raises after the rest of the batch has been added; with raise_on_error=False rc is -5 and the record shows in its status.
        The handle stays usable either way."""
        if self._h is None:
            raise _lib.S5GpuError("contrast handle: already closed")
        n = len(records)
        vp = C.c_void_p
        rb = [bytes(x) for x in records]
        rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
        rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
        rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
        map_rows, rows, status = np.zeros(n, dtype=MAP_ROW), np.zeros(n, dtype=_extend.EXT_ROW), np.zeros(n, dtype=np.int32)
        rc = _lib.lib().s5gpu_contrast_add_batch(self._h, int(side), n, rec_p, rl, rec_method, sig_method, map_rows.ctypes.data_as(vp), rows.ctypes.data_as(vp),
                                                 status.ctypes.data_as(vp))
        if rc != 0 and (raise_on_error or rc != ERR_DATA):
            check(rc, "s5gpu_contrast_add_batch")
        return rc, map_rows, rows, status

    def close(self):
        if self._h is None:
            raise _lib.S5GpuError("contrast handle: already closed")
        vp = C.c_void_p
        a, b = (np.zeros(_pileup.acc_bytes(self.R), dtype=np.uint8) for _ in range(2))
        rows = np.zeros(self.R, dtype=CONTRAST_ROW)
        h, self._h = self._h, None
        check(_lib.lib().s5gpu_contrast_close(h, a.ctypes.data_as(vp), b.ctypes.data_as(vp), rows.ctypes.data_as(vp)), "s5gpu_contrast_close")
        return rows, _pileup.from_bytes(a), _pileup.from_bytes(b)

    def close_folded(self, cls, K):
        """close(), with both sides' table and histogram folded onto K classes on the device first and the comparison made over the K rows
        (s5gpu_contrast_close_folded, §4.26): cls a uint32 class per reference column (RefSeq.classes()).  The handle ends whatever happens."""
        if self._h is None:
            raise _lib.S5GpuError("contrast handle: already closed")
        vp = C.c_void_p
        c = np.ascontiguousarray(cls, dtype=np.uint32)
        h, self._h = self._h, None
        if c.shape != (self.R,) or hist_bytes(K) == 0:
            _lib.lib().s5gpu_contrast_close(h, None, None, None)
            raise ValueError("close_folded: cls holds a class per column (%d), K is 1 .. 2^22" % self.R)
        a, b = (np.zeros(_pileup.acc_bytes(K), dtype=np.uint8) for _ in range(2))
        rows = np.zeros(int(K), dtype=CONTRAST_ROW)
        check(_lib.lib().s5gpu_contrast_close_folded(h, c.ctypes.data_as(vp), int(K), a.ctypes.data_as(vp), b.ctypes.data_as(vp), rows.ctypes.data_as(vp)),
              "s5gpu_contrast_close_folded")
        return rows, _pileup.from_bytes(a), _pileup.from_bytes(b)

    def abandon(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().s5gpu_contrast_close(h, None, None, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.abandon()
        return False


def file_contrast(a, b, ref_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, min_depth=1, q0=Q0, shift=SHIFT, emax=None, tile_rows=None, band=None,
                  raise_on_corrupt=True, refine=False, iters=None, slope=None):
    """The positions of two .blow5 files against the levels of ref_path (one number per line) as a CONTRAST_LINE array, a row per reference
    position whose depth is at least min_depth in both.  Runs the s5contrast tool (examples/s5contrast.c), `batch` records per device call.
    A corrupt record raises; with raise_on_corrupt=False it is left out.  refine=True: --refine, with iters and slope as in extend.file_extend."""
    if not os.path.exists(S5CONTRAST):
        _build.build()
    cmd = [S5CONTRAST, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin)), "--min-depth", str(int(min_depth)),
           "--q0", str(int(q0)), "--shift", str(int(shift))]
    cmd += (["--rna"] if rna else []) + (["--max-events", str(int(emax))] if emax is not None else [])
    cmd += (["--tile", str(int(tile_rows))] if tile_rows is not None else []) + (["--band", str(int(band))] if band is not None else [])
    if refine:
        cmd += ["--refine"] + (["--iters", str(int(iters))] if iters is not None else [])
        cmd += ["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []
    cmd += [os.fspath(ref_path), os.fspath(a), os.fspath(b)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5contrast %s %s failed (exit %d): %s" % (a, b, p.returncode, p.stderr.decode(errors="replace").strip()))
    lines = []
    for ln in p.stdout.split(b"\n"):
        if ln:
            f = ln.split(b"\t")
            lines.append(tuple(int(f[k]) for k in range(6)) + (float(f[6]), float(f[7]), float(f[8]), int(f[9]), float(f[10]), int(f[11]), int(f[12])))
    return np.array(lines, dtype=CONTRAST_LINE).reshape(-1)
