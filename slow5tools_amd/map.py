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
  sdtw2_dev, map2_dev, read_map2 : the same with the second-best hit and a mapping quality beside each row (MAP_SECOND; §4.19)
  RefSeq      : a reference made from sequences and a k-mer model on the host, both strands, and the way back from columns to positions

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
# ... and of s5gpu_map_second_t: the runner-up of a read (cost2 = NO_COST and end2 = -1: none) and the mapping quality 0 .. 60
MAP_SECOND = np.dtype([("cost2", "<u4"), ("end2", "<i4"), ("mapq", "<u4"), ("zero", "<u4")])
assert MAP_SECOND.itemsize == 16
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


# ---------------------------------------------------------------------------------------------------------------- the second-best hit (§4.19)

def default_bshift(qmax=QMAX):
    """the smallest block shift in 6 .. 30 whose block of 2^shift columns holds qmax columns"""
    return max(6, (int(qmax) - 1).bit_length())


def sdtw2_dev(queries, qlen, ref_tensor, want_start=False, bshift=None):
    """k_sdtw2: sdtw_dev and the second-best hit in the same pass -> (rows, second): rows what sdtw_dev returns, second an [n, 4] int32 tensor,
    columns cost2 (as uint32 bits), end2, mapq, 0.  bshift: blocks of 2^bshift columns (6 .. 30; default: the pitch fits a block).  Asynchronous,
    on the current stream."""
    import torch

    if queries.dtype != torch.int16 or ref_tensor.dtype != torch.int16 or queries.dim() != 2 or ref_tensor.dim() != 1:
        raise ValueError("sdtw2_dev: queries [n, qpitch] and ref_tensor [R] are int16 tensors")
    queries, ref_tensor, qlen = queries.contiguous(), ref_tensor.contiguous(), qlen.to(torch.int32).contiguous()
    n, dev = int(queries.shape[0]), queries.device
    bshift = default_bshift(queries.shape[1]) if bshift is None else int(bshift)
    out = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    out2 = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    check(_lib.lib().s5gpu_sdtw2_dev(n, queries.data_ptr(), int(queries.shape[1]), qlen.data_ptr(), ref_tensor.data_ptr() if ref_tensor.numel() else None,
                                     int(ref_tensor.numel()), 1 if want_start else 0, bshift, out.data_ptr(), out2.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_sdtw2_dev")
    return out[:n], out2[:n]


def _ref_of(ref, clip, who):
    """the int16 reference of a call: an array, or a RefSeq, whose walls hold only for the clip it was built with"""
    if isinstance(ref, RefSeq):
        if int(clip) != ref.clip:
            raise ValueError("%s: clip %d, but the reference was built with clip %d (its walls are sized for that)" % (who, int(clip), ref.clip))
        return ref.ref
    return ref


def map2_dev(dec, ref, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP, want_start=False, bshift=None):
    """map_dev with the second-best hit -> (MAP_ROW array, MAP_SECOND array, status) on the host.  ref: an int16 numpy array, a device tensor
    or a RefSeq."""
    import torch

    ref = _ref_of(ref, clip, "map2_dev")
    rows, first = _events.events_dev(dec, event_params, "raw")
    fst = dec.t_fields.view(torch.int32).view(-1, 16)[:dec.n, 0].contiguous()
    q, ql, st = queries_dev(rows, first, fst, skip, qmax, qmin, scale, clip)
    r = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.int16))
    out, out2 = sdtw2_dev(q, ql, r.to(dec.dev), want_start, bshift)
    return (out.cpu().numpy().view(MAP_ROW).reshape(-1).copy(), out2.cpu().numpy().view(MAP_SECOND).reshape(-1).copy(), st.cpu().numpy().copy())


def read_map2(records, ref, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, event_params=DNA, skip=SKIP, qmax=QMAX, qmin=QMIN, scale=SCALE, clip=CLIP,
              want_start=False, bshift=None, raise_on_error=True):
    """read_map with the second-best hit, through s5gpu_map2_batch -> (MAP_ROW array, MAP_SECOND array, status).  ref: an int16 array or a
    RefSeq.  A corrupt record raises; with raise_on_error=False it has its status and empty rows, the others are valid."""
    L = _lib.lib()
    n = len(records)
    ep, mp = _events._params(event_params), _params(skip, qmax, qmin, scale, clip, want_start)
    r = np.ascontiguousarray(_ref_of(ref, clip, "read_map2"), dtype=np.int16)
    bshift = default_bshift(qmax) if bshift is None else int(bshift)
    vp = C.c_void_p
    rb = [bytes(x) for x in records]
    rbuf = [C.create_string_buffer(x, max(len(x), 1)) for x in rb]
    rec_p = (vp * max(n, 1))(*[C.addressof(b) for b in rbuf])
    rl = (C.c_size_t * max(n, 1))(*[len(x) for x in rb])
    rows = np.zeros(n, dtype=MAP_ROW)
    second = np.zeros(n, dtype=MAP_SECOND)
    status = np.zeros(n, dtype=np.int32)
    rc = L.s5gpu_map2_batch(n, rec_p, rl, rec_method, sig_method, C.byref(ep), C.byref(mp), r.ctypes.data_as(vp), len(r), bshift, rows.ctypes.data_as(vp),
                            second.ctypes.data_as(vp), status.ctypes.data_as(vp))
    if rc != 0 and (raise_on_error or rc != -5):
        check(rc, "s5gpu_map2_batch")
    return rows, second, status


class RefSeq:
    """A reference squiggle made from sequences and a k-mer model on the host (s5gpu_refseq_*, §4.19): per contig the forward levels, then
    (DNA, strands=2) those of the reverse complement, or (rna) the forward levels reversed; all quantised together, walls of -32768 between
    the segments.

      RefSeq(fasta=path, model=path)                          from files
      RefSeq(contigs=[(name, sequence), ...], levels=array)   from memory: levels the 4^k model levels in k-mer rank order

      .ref        the int16 reference (a numpy array): what read_map2, read_align and Pileup take
      .segments   a list of (contig, name, strand, offset, Lk), strand '+' or '-'
      .contigs    a list of (name, bases, Lk); Lk = 0: shorter than k, no segment
      .k, .wall, .clip
      .classes()  the k-mer rank of every column, and 4^k: what model.fold_dev and close_folded take (§4.26)
      .quant      (mu, sd, scale): the way back from a quantised level to the model's units
    """

    def __init__(self, fasta=None, model=None, contigs=None, levels=None, strands=2, rna=False, scale=SCALE, clip=CLIP):
        L = _lib.lib()
        self._h = None
        if (fasta is None) == (contigs is None) or (fasta is None) != (model is None) or (contigs is None) != (levels is None):
            raise ValueError("RefSeq: fasta and model, or contigs and levels")
        if fasta is not None:
            h = L.s5gpu_refseq_open(os.fsencode(fasta), os.fsencode(model), int(strands), 1 if rna else 0, float(scale), int(clip))
        else:
            lv = np.ascontiguousarray(levels, dtype=np.float32)
            k = (max(len(lv), 1).bit_length() - 1) // 2
            if lv.ndim != 1 or k < 1 or len(lv) != 4 ** k:
                raise ValueError("RefSeq: levels holds 4^k values, k in 1 .. 10")
            names = [n if isinstance(n, bytes) else str(n).encode() for n, s in contigs]
            seqs = [s if isinstance(s, bytes) else str(s).encode() for n, s in contigs]
            m = max(len(names), 1)
            name_p, seq_p = (C.c_char_p * m)(*names), (C.c_char_p * m)(*seqs)
            lens = (C.c_size_t * m)(*[len(s) for s in seqs])
            h = L.s5gpu_refseq_build(len(names), name_p, seq_p, lens, lv.ctypes.data_as(C.c_void_p), k, int(strands), 1 if rna else 0, float(scale), int(clip))
        if not h:
            raise _lib.S5GpuError("RefSeq: " + L.s5gpu_last_error().decode(errors="replace"))
        self._h = C.c_void_p(h)
        R, k, W, cl = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        p = L.s5gpu_refseq_ref(self._h, C.byref(R))
        check(L.s5gpu_refseq_params(self._h, C.byref(k), C.byref(W), C.byref(cl)), "s5gpu_refseq_params")
        self.ref = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int16)), (R.value,)).copy()
        self.k, self.wall, self.clip = k.value, W.value, cl.value
        self.segments, self.contigs = [], []
        for i in range(L.s5gpu_refseq_n_segments(self._h)):
            s = _lib.RefSeqSegment()
            check(L.s5gpu_refseq_segment(self._h, i, C.byref(s)), "s5gpu_refseq_segment")
            self.segments.append((s.contig, s.name.decode(errors="replace"), chr(s.strand), s.offset, s.Lk))
        for i in range(L.s5gpu_refseq_n_contigs(self._h)):
            nm, ln, lk = C.c_char_p(), C.c_uint64(), C.c_uint32()
            check(L.s5gpu_refseq_contig(self._h, i, C.byref(nm), C.byref(ln), C.byref(lk)), "s5gpu_refseq_contig")
            self.contigs.append((nm.value.decode(errors="replace"), ln.value, lk.value))

    def locate(self, cols):
        """reference columns -> a list of (contig, strand, pos): the contig's index, '+' or '-', the 0-based start of the column's k-mer on the
        forward strand; a wall column: (-1, 'wall', -1)"""
        L, out, loc = _lib.lib(), [], _lib.RefSeqLoc()
        for c in np.asarray(cols, dtype=np.int64).reshape(-1):
            rc = L.s5gpu_refseq_locate(self._h, int(c) if 0 <= c < 2 ** 32 else 0xFFFFFFFF, C.byref(loc))
            if rc == _lib.REFSEQ_WALL:
                out.append((-1, "wall", -1))
            else:
                check(rc, "s5gpu_refseq_locate")
                out.append((loc.contig, chr(loc.strand), loc.pos))
        return out

    def classes(self):
        """(cls, K): a uint32 class per column of .ref, the base-4 rank of the k-mer the column shows (the rank whose level it took), and
        K = 4^k; 0xFFFFFFFF for a wall column and for a k-mer that holds a letter other than ACGT (s5gpu_refseq_classes, §4.26)"""
        cls, K = np.zeros(len(self.ref), dtype=np.uint32), C.c_uint32()
        check(_lib.lib().s5gpu_refseq_classes(self._h, cls.ctypes.data_as(C.c_void_p), C.byref(K)), "s5gpu_refseq_classes")
        return cls, K.value

    @property
    def quant(self):
        """(mu, sd, scale) of the quantiser over all segments' levels: a quantised level q stands for mu + (sd / scale) q"""
        mu, sd, sc = C.c_double(), C.c_double(), C.c_double()
        check(_lib.lib().s5gpu_refseq_quant(self._h, C.byref(mu), C.byref(sd), C.byref(sc)), "s5gpu_refseq_quant")
        return mu.value, sd.value, sc.value

    def spans(self, rows):
        """the (start, end) of MAP_ROW rows -> a list of (contig, strand, pos_lo, pos_hi), pos_lo <= pos_hi the first and last k-mer start on
        the forward strand; None for a row without a query or without a start, and for a span that is not inside one segment"""
        out = []
        for r in np.asarray(rows).reshape(-1):
            if r["qlen"] == 0 or r["start"] < 0 or r["end"] < 0:
                out.append(None)
                continue
            (c0, s0, p0), (c1, s1, p1) = self.locate([r["start"], r["end"]])
            out.append((c0, s0, min(p0, p1), max(p0, p1)) if (c0, s0) == (c1, s1) and c0 >= 0 else None)
        return out

    def close(self):
        if self._h is not None:
            _lib.lib().s5gpu_refseq_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
