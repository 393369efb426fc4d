"""model: the pileup folded onto k-mers, and a k-mer level table re-estimated from it (include/slow5gpu.h "model", docs/codecs.md §4.26).

The tables of pileup and contrast are indexed by reference column.  A fold adds the columns that share a class -- cls[j] < K, the rank of the
k-mer column j shows (map.RefSeq.classes()) -- into an ordinary table (histogram) of K columns on the device: pileup.to_host,
contrast.contrast_dev and the line printers take it as it stands.  Every member is an integer sum, minimum or maximum.  From the folded
sums of a whole-read pileup (refined, so that they are in the reference's units) a level table is estimated: what signal-level tools call
a round of `train`.

  fold_dev      : an accumulator tensor of R columns and a class per column -> an accumulator of K columns (k_pile_fold)
  hist_fold_dev : the same for a histogram tensor (k_pile_hist_fold)
  refused       : did a fold refuse (2^32 cells or more, heads that disagree)?  from the (total, cols) or (head, counts) of the output
  solve         : a folded table, the RefSeq that made the reference and the current levels -> a KMER_ROW array (s5gpu_kmer_model_solve)
  write_model   : a KMER_ROW array -> a model file that s5gpu_kmer_model_load (map.RefSeq(model=...)) reads back
  read_model    : that file -> (k, a MODEL_LINE array)
  file_model    : a .blow5 file, a FASTA file and a model -> the new model file, through the s5model tool
  Pileup.close_folded, PileupWhole.close_folded, Contrast.close_folded : the handles' closes with the fold in front of the download

Two limits of the estimate: queries are clamped to +-clip, so a k-mer near +-4 sd is biased inwards; and the estimate is in the units of
the table that made the reference, so a round changes the table's shape and not its overall scale.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from . import contrast as _contrast
from . import pileup as _pileup
from ._lib import FOLD_NONE, FOLD_REFUSED, check  # noqa: F401  (FOLD_NONE: for callers)
from .map import QMAX, QMIN, SKIP

KMER_ROW = _lib.KmerRow
# a line of the tool
MODEL_LINE = np.dtype([("kmer", "S10"), ("level_mean", "<f8"), ("level_stdv", "<f8"), ("cells", "<u4"), ("occurrences", "<u4"), ("dwell", "<f8"), ("kept", "<u4")])
MIN_CELLS = 30
S5MODEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5model")


def _stream(dev):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _cls_tensor(cls, R, dev):
    import torch

    t = cls if isinstance(cls, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint32).view(np.int32))
    if t.dim() != 1 or int(t.numel()) != R or t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise ValueError("cls holds a 32-bit class per column (%d)" % R)
    return t.to(dev).contiguous()


def fold_dev(acc, cls, K, out=None):
    """k_pile_fold: acc, an accumulator tensor of pileup with R columns, added into an accumulator of K columns by the classes cls (a uint32
    numpy array or a 32-bit device tensor of R entries; a class >= K drops its column).  out: the accumulator to add to (new_acc(K) when
    None): the fold adds, so several inputs may go into one output.  Asynchronous, on the current stream.  Returns out."""
    import torch

    if acc.dtype != torch.uint8 or acc.dim() != 1 or int(acc.numel()) < 64 + 48 or (int(acc.numel()) - 64) % 48:
        raise ValueError("fold_dev: not an accumulator tensor")
    R, dev = (int(acc.numel()) - 64) // 48, acc.device
    c = _cls_tensor(cls, R, dev)
    if out is None:
        out = _pileup.new_acc(K, dev)
    elif out.dtype != torch.uint8 or int(out.numel()) != _pileup.acc_bytes(K):
        raise ValueError("fold_dev: out is not an accumulator of %d columns" % K)
    check(_lib.lib().s5gpu_pileup_fold_dev(acc.data_ptr(), R, c.data_ptr(), int(K), out.data_ptr(), _stream(dev)), "s5gpu_pileup_fold_dev")
    c.record_stream(torch.cuda.current_stream(dev))
    return out


def hist_fold_dev(hist, cls, K, out=None, q0=None, shift=None):
    """k_pile_hist_fold: the same for a histogram tensor of contrast.  out None: a new histogram of K columns with the input's q0 and shift
    (one small download to read them) unless both are given."""
    import torch

    R, dev = _contrast._columns(hist), hist.device
    c = _cls_tensor(cls, R, dev)
    if out is None:
        if q0 is None or shift is None:
            head = hist[:64].cpu().numpy().view(_contrast.HIST_HEAD)[0]
            q0, shift = int(head["q0"]), int(head["shift"])
        out = _contrast.new_hist(K, q0, shift, dev)
    elif out.dtype != torch.uint8 or int(out.numel()) != _contrast.hist_bytes(K):
        raise ValueError("hist_fold_dev: out is not a histogram of %d columns" % K)
    check(_lib.lib().s5gpu_pile_hist_fold_dev(hist.data_ptr(), R, c.data_ptr(), int(K), out.data_ptr(), _stream(dev)), "s5gpu_pile_hist_fold_dev")
    c.record_stream(torch.cuda.current_stream(dev))
    return out


def refused(head):
    """head: the total of pileup.to_host or the head of contrast.hist_to_host of a fold's output -> did a fold into it add nothing?"""
    r = head["reserved"]
    return bool(int(np.asarray(r).reshape(-1)[0]) & FOLD_REFUSED)


def solve(acc_folded, refseq, levels_in, min_cells=MIN_CELLS):
    """The estimate (s5gpu_kmer_model_solve; host arithmetic in double): acc_folded a (total, cols) pair of K = 4^k columns or the bytes of
    one, refseq the map.RefSeq whose reference the pileup ran against (or its (mu, sd, scale)), levels_in the 4^k levels that made it ->
    a KMER_ROW array.  A k-mer with fewer than min_cells cells keeps its level (kept = 1)."""
    if isinstance(acc_folded, tuple):
        total, cols = acc_folded
        raw = np.concatenate([np.frombuffer(np.asarray(total).tobytes(), dtype=np.uint8), np.frombuffer(np.ascontiguousarray(cols).tobytes(), dtype=np.uint8)])
    else:
        raw = np.frombuffer(bytes(acc_folded), dtype=np.uint8)
    K = (len(raw) - 64) // 48
    mu, sd, scale = refseq.quant if hasattr(refseq, "quant") else refseq
    lv = np.ascontiguousarray(levels_in, dtype=np.float32)
    if len(raw) != 64 + 48 * K or K < 1 or lv.shape != (K,):
        raise ValueError("solve: a folded table of K columns and K levels")
    raw = np.ascontiguousarray(raw)
    rows = np.zeros(K, dtype=KMER_ROW)
    vp = C.c_void_p
    check(_lib.lib().s5gpu_kmer_model_solve(raw.ctypes.data_as(vp), K, float(mu), float(sd), float(scale), int(min_cells), lv.ctypes.data_as(vp),
                                            rows.ctypes.data_as(vp)), "s5gpu_kmer_model_solve")
    return rows


def kmer_of(rank, k):
    """the k-mer of a base-4 rank: A, C, G, T = 0 .. 3, the first base most significant"""
    return "".join("ACGT"[(int(rank) >> (2 * (k - 1 - b))) & 3] for b in range(k))


def write_model(path, k, rows, occurrences=None, reads_used=0, rounds=1):
    """A KMER_ROW array of 4^k rows -> the file the s5model tool writes: a `#` line (k, the reads used, the rounds), the column names, and
    per k-mer in rank order kmer, level_mean (the level rounded to float32, as %.9g: it survives that), level_stdv, cells, occurrences, dwell, kept.
    s5gpu_kmer_model_load reads it back; it ignores the columns behind level_mean."""
    rows = np.asarray(rows)
    if rows.shape != (4 ** int(k),):
        raise ValueError("write_model: 4^k rows")
    occ = np.zeros(len(rows), dtype=np.uint32) if occurrences is None else np.asarray(occurrences)
    with open(path, "w") as fh:
        fh.write("# s5model k=%d reads_used=%d rounds=%d\nkmer\tlevel_mean\tlevel_stdv\tcells\toccurrences\tdwell\tkept\n" % (int(k), int(reads_used), int(rounds)))
        for r in range(len(rows)):
            x = rows[r]
            fh.write("%s\t%.9g\t%.6g\t%d\t%d\t%.6g\t%d\n" % (kmer_of(r, k), float(np.float32(x["level"])), float(x["stdv"]), int(x["cells"]), int(occ[r]), float(x["dwell"]),
                                                             int(x["kept"])))


def occurrences(cls, K):
    """how many columns show each class: the `occurrences` column of the tool"""
    c = np.asarray(cls, dtype=np.uint32)
    return np.bincount(c[c < K], minlength=int(K)).astype(np.uint32)


def read_model(path):
    """a model file of write_model or s5model -> (k, a MODEL_LINE array in file order); columns a plain `kmer level` file lacks are 0"""
    out = []
    with open(path, "rb") as fh:
        for ln in fh:
            ln = ln.strip()
            if not ln or ln.startswith(b"#") or ln.startswith(b"kmer"):
                continue
            f = ln.split()
            f += [b"0"] * (7 - len(f))
            out.append((f[0], float(f[1]), float(f[2]), int(f[3]), int(f[4]), float(f[5]), int(f[6])))
    t = np.array(out, dtype=MODEL_LINE).reshape(-1)
    return (len(out[0][0]) if out else 0), t


def file_model(path, fasta, model, out_path, batch=4096, rna=False, skip=SKIP, qmax=QMAX, qmin=QMIN, emax=None, tile_rows=None, band=None, refine=False,
               refine_iters=None, slope=None, iters=1, min_cells=MIN_CELLS, fwd_only=False, raise_on_corrupt=True):
    """`iters` rounds of the estimate on a .blow5 file, from the sequences of `fasta` and the table `model`, into out_path -> (k, a MODEL_LINE
    array).  Runs the s5model tool (examples/s5model.c), `batch` records per device call.  refine=True: --refine (with refine_iters and slope
    as iters and slope of extend.file_extend): the sums are then in the reference's units, which the estimate assumes."""
    if not os.path.exists(S5MODEL):
        _build.build()
    cmd = [S5MODEL, "-K", str(int(batch)), "--skip", str(int(skip)), "--events", str(int(qmax)), "--min-events", str(int(qmin)), "--iters", str(int(iters)),
           "--min-cells", str(int(min_cells))]
    cmd += (["--rna"] if rna else []) + (["--fwd-only"] if fwd_only else []) + (["--max-events", str(int(emax))] if emax is not None else [])
    cmd += (["--tile", str(int(tile_rows))] if tile_rows is not None else []) + (["--band", str(int(band))] if band is not None else [])
    if refine:
        cmd += ["--refine"] + (["--refine-iters", str(int(refine_iters))] if refine_iters is not None else [])
        cmd += ["--slope", "%.17g,%.17g" % (float(slope[0]), float(slope[1]))] if slope is not None else []
    cmd += ["--fasta", os.fspath(fasta), "--model", os.fspath(model), "-o", os.fspath(out_path), os.fspath(path)]
    p = subprocess.run(cmd, capture_output=True)
    if p.returncode != 0 and (raise_on_corrupt or p.returncode != 1):
        raise _lib.S5GpuError("s5model %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    return read_model(out_path)
