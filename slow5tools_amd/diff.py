"""diff: where and by how much the reads of two files differ, compared on the device (include/slow5gpu.h "diff", docs/codecs.md §4.14).

  pair_diffs : two lists of records (pair i = record i of each) -> (rows, accumulator): numpy records of dtype SIG_DIFF and DIFF_ACC
  Handle     : the per-file handle behind it (s5gpu_diff_add_batch); close() makes the one download of the accumulator
  diff_dev   : k_sig_diff on what two press.decode_to_device calls left on the device, over any list of pairs
  file_diff  : two .blow5 files -> what the s5diff tool prints, parsed

Every member is an integer sum, maximum or count: numpy over the decoded samples is the exact oracle.  There is no host implementation of the
metrics here: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from ._lib import DIFF_ACC, SIG_DIFF, check

ERR_DATA = -5
S5DIFF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5diff")


def _rec_arrays(records):
    """(keep-alive buffers, void*[n], size_t[n]) of a list of records"""
    n = len(records)
    rb = [bytes(r) for r in records]
    bufs = [C.create_string_buffer(r, max(len(r), 1)) for r in rb]
    return bufs, (C.c_void_p * n)(*[C.addressof(b) for b in bufs]), (C.c_size_t * n)(*[len(r) for r in rb])


class Handle:
    """One file pair's accumulator and side-A buffers on the first device in use."""

    def __init__(self):
        self._h = _lib.lib().s5gpu_diff_open()
        if not self._h:
            check(-4, "s5gpu_diff_open")

    def add(self, recs_a, methods_a, recs_b, methods_b, raise_on_error=True):
        """Pair i is record i of each list (bytes without the u64 prefix); methods_x = (rec_method, sig_method).  Returns (rows, status_a,
        status_b).  A corrupt record raises after the other pairs have been compared and its pair counted in n_failed; with
        raise_on_error=False it only shows in its row (flags FAILED) and status."""
        if self._h is None:
            raise _lib.S5GpuError("diff handle: already closed")
        n = len(recs_a)
        if len(recs_b) != n:
            raise ValueError("diff: %d records against %d" % (n, len(recs_b)))
        rows = np.zeros(n, dtype=SIG_DIFF)
        st_a, st_b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        if n:
            vp = C.c_void_p
            keep_a, pa, la = _rec_arrays(recs_a)
            keep_b, pb, lb = _rec_arrays(recs_b)
            rc = _lib.lib().s5gpu_diff_add_batch(self._h, n, pa, la, methods_a[0], methods_a[1], pb, lb, methods_b[0], methods_b[1],
                                                 rows.ctypes.data_as(vp), st_a.ctypes.data_as(vp), st_b.ctypes.data_as(vp))
            if rc != 0 and (raise_on_error or rc != ERR_DATA):
                check(rc, "s5gpu_diff_add_batch")
        return rows, st_a, st_b

    def close(self):
        out = np.zeros(1, dtype=DIFF_ACC)
        h, self._h = self._h, None
        if h is not None:
            check(_lib.lib().s5gpu_diff_close(h, out.ctypes.data_as(C.c_void_p)), "s5gpu_diff_close")
        return out[0]

    def abandon(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().s5gpu_diff_close(h, None)


def pair_diffs(recs_a, methods_a, recs_b, methods_b, batch=None):
    """(rows, accumulator) of the pairs (recs_a[i], recs_b[i]), `batch` pairs per device call (all at once when None)."""
    n = len(recs_a)
    step = n if not batch else int(batch)
    h = Handle()
    try:
        parts = [h.add(recs_a[lo:lo + step], methods_a, recs_b[lo:lo + step], methods_b)[0] for lo in range(0, n, max(step, 1))]
    except Exception:
        h.abandon()
        raise
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=SIG_DIFF)), h.close()


def new_acc(device="cuda:0"):
    """an empty accumulator as a uint8 tensor on the device (s5gpu_diff_acc_reset_dev)"""
    import torch

    dev = torch.device(device)
    t = torch.zeros(DIFF_ACC.itemsize, dtype=torch.uint8, device=dev)
    check(_lib.lib().s5gpu_diff_acc_reset_dev(t.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_diff_acc_reset_dev")
    return t


class _Side:
    """s5gpu_diff_side_t of a press.DecodedDev, with the device arrays it points to kept alive"""

    def __init__(self, dec, payload):
        import torch

        d = dec.t_desc.cpu().numpy().view(_lib.REC_DESC)[:dec.n]
        self.t_off = torch.from_numpy(d["sig_off"].astype(np.uint64).view(np.int64).copy()).to(dec.dev)
        self.t_cap = torch.from_numpy(d["sig_cap"].astype(np.uint32).view(np.int32).copy()).to(dec.dev)
        self.c = _lib.DiffSide()
        self.c.n, self.c.sig, self.c.sig_off, self.c.sig_cap, self.c.fields = dec.n, dec.t_sig.data_ptr(), self.t_off.data_ptr(), self.t_cap.data_ptr(), dec.t_fields.data_ptr()
        if payload:
            self.t_poff = torch.from_numpy(d["pay_off"].astype(np.uint64).view(np.int64).copy()).to(dec.dev)
            self.t_pcap = torch.from_numpy(d["pay_cap"].astype(np.uint32).view(np.int32).copy()).to(dec.dev)
            self.c.payload, self.c.pay_off, self.c.pay_cap = dec.t_scr.data_ptr(), self.t_poff.data_ptr(), self.t_pcap.data_ptr()


def diff_dev(dec_a, dec_b, pair_a, pair_b, acc_tensor=None, payload=False, want_rows=True):
    """k_sig_diff over the pairs (pair_a[p], pair_b[p]) of two press.decode_to_device results.  payload=True: both were decoded with
    no_payload=False and ID / AUX are compared.  acc_tensor (new_acc()) receives the pairs' sums when given.  Returns the rows as a numpy array
    of dtype SIG_DIFF (None when want_rows is False); the stream is synchronised."""
    import torch

    dev = dec_a.dev
    pa = torch.from_numpy(np.asarray(pair_a, dtype=np.uint32).view(np.int32).copy()).to(dev)
    pb = torch.from_numpy(np.asarray(pair_b, dtype=np.uint32).view(np.int32).copy()).to(dev)
    if pa.numel() != pb.numel():
        raise ValueError("diff_dev: %d indices against %d" % (pa.numel(), pb.numel()))
    n = pa.numel()
    A, B = _Side(dec_a, payload), _Side(dec_b, payload)
    rows = torch.zeros(max(n, 1) * SIG_DIFF.itemsize, dtype=torch.uint8, device=dev) if want_rows else None
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(_lib.lib().s5gpu_signal_diff_dev(n, pa.data_ptr(), pb.data_ptr(), C.byref(A.c), C.byref(B.c), rows.data_ptr() if want_rows else None,
                                           acc_tensor.data_ptr() if acc_tensor is not None else None, st), "s5gpu_signal_diff_dev")
    torch.cuda.synchronize(dev)          # the index and descriptor tensors die with this frame
    return rows.cpu().numpy().view(SIG_DIFF)[:n].copy() if want_rows else None


def to_numpy(acc_tensor):
    """the accumulator tensor as a numpy record"""
    return acc_tensor.cpu().numpy().view(DIFF_ACC)[0].copy()


def file_diff(path_a, path_b, batch=4096, tol=None, hist=None):
    """Runs the s5diff tool (examples/s5diff.c) on two .blow5 files, `batch` records per device call.  Returns a dict: "exit" (0 no flagged pair
    and no unpaired id, or everything within tol; 1 otherwise), "pairs" (one dict per flagged pair, A's order), "only_in_a", "only_in_b",
    "header_differs", "aux_layout_differs" and "summary" (the '#' lines by name, as lists of strings).  Any error of the tool raises."""
    if not os.path.exists(S5DIFF):
        _build.build()
    cmd = [S5DIFF, "-K", str(int(batch))]
    if tol is not None:
        cmd += ["--tol", str(int(tol))]
    if hist is not None:
        cmd += ["--hist", os.fspath(hist)]
    p = subprocess.run(cmd + [os.fspath(path_a), os.fspath(path_b)], capture_output=True)
    if p.returncode not in (0, 1):
        raise _lib.S5GpuError("s5diff %s %s failed (exit %d): %s" % (path_a, path_b, p.returncode, p.stderr.decode(errors="replace").strip()))
    lines = p.stdout.decode(errors="replace").split("\n")
    if lines[0] != "#s5diff\t1":
        raise _lib.S5GpuError("s5diff: unexpected first line %r" % lines[0])
    res = {"exit": p.returncode, "pairs": [], "only_in_a": [], "only_in_b": [], "header_differs": False, "aux_layout_differs": False, "summary": {}}
    for ln in lines[1:]:
        f = ln.split("\t")
        if not ln:
            continue
        if ln.startswith("#"):
            res["summary"][f[0][1:]] = f[1:]
        elif f[0] == "header":
            res["header_differs"] = True
        elif f[0] == "aux-layout":
            res["aux_layout_differs"] = True
        elif f[0] in ("only-in-a", "only-in-b"):
            res[f[0].replace("-", "_")].append(f[1])
        else:
            res["pairs"].append(dict(zip(("read_id", "flags", "n_a", "n_b", "n_diff", "first_diff", "max_abs", "max_at", "rmse"), f)))
    return res
