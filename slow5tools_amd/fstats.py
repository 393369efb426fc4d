"""stats: what is in a whole file's signal, accumulated on the device while the batches stream through
(include/slow5gpu.h "stats", docs/codecs.md §4.13).

  file_stats  : a .blow5 / .slow5 file -> the accumulator, a numpy record of dtype FILE_STATS
  accumulate  : records -> a per-file handle (s5gpu_file_stats_add_stream); Handle.close() makes the one download
  accum_dev   : k_file_stats on what press.decode_to_device left on the device, into an accumulator tensor

Every member is an integer sum, minimum, maximum, OR or AND: numpy over the decoded samples is the exact oracle.
"""
import ctypes as C
import struct

import numpy as np

from . import _lib
from ._lib import FILE_STATS, REC_NONE, REC_ZLIB, SIG_NONE, SIG_SVB_ZD, check

ERR_DATA = -5


class Handle:
    """One file's accumulator on the first device in use.  close() -> the numpy record (and the end of the handle)."""

    def __init__(self):
        self._h = _lib.lib().s5gpu_file_stats_open()
        if not self._h:
            check(-4, "s5gpu_file_stats_open")

    def add(self, records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True):
        """Adds a batch of records (bytes without the u64 prefix); returns their decode statuses (int32).  A corrupt record raises after the
        rest of the batch has been added and the record counted in n_failed; with raise_on_error=False it only shows in its status."""
        if self._h is None:
            raise _lib.S5GpuError("file_stats handle: already closed")
        n = len(records)
        status = np.zeros(n, dtype=np.int32)
        if n:
            pos, parts, at = np.zeros(n, dtype=np.uint64), [], 0
            for i, r in enumerate(records):
                r = bytes(r)
                parts.append(struct.pack("<Q", len(r)) + r)
                pos[i] = at + 8
                at += 8 + len(r)
            chunk = np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8)
            lens = np.array([len(r) for r in records], dtype=np.uint32)
            vp = C.c_void_p
            rc = _lib.lib().s5gpu_file_stats_add_stream(self._h, n, chunk.ctypes.data_as(vp), at, pos.ctypes.data_as(vp), lens.ctypes.data_as(vp),
                                                        rec_method, sig_method, status.ctypes.data_as(vp))
            if rc != 0 and (raise_on_error or rc != ERR_DATA):
                check(rc, "s5gpu_file_stats_add_stream")
        return status

    def close(self):
        out = np.zeros(1, dtype=FILE_STATS)
        h, self._h = self._h, None
        if h is not None:
            check(_lib.lib().s5gpu_file_stats_close(h, out.ctypes.data_as(C.c_void_p)), "s5gpu_file_stats_close")
        return out[0]

    def abandon(self):
        h, self._h = self._h, None
        if h is not None:
            _lib.lib().s5gpu_file_stats_close(h, None)


def accumulate(records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, handle=None):
    """Adds a batch of records to `handle` (a new Handle when None) and returns the handle: call close() on it for the result."""
    h = handle if handle is not None else Handle()
    try:
        h.add(records, rec_method, sig_method)
    except Exception:
        if handle is None:
            h.abandon()
        raise
    return h


def new_acc(device="cuda:0"):
    """an empty accumulator as a uint8 tensor on the device (s5gpu_file_stats_reset_dev)"""
    import torch

    dev = torch.device(device)
    t = torch.zeros(FILE_STATS.itemsize, dtype=torch.uint8, device=dev)
    check(_lib.lib().s5gpu_file_stats_reset_dev(t.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "s5gpu_file_stats_reset_dev")
    return t


def accum_dev(dec, acc_tensor):
    """k_file_stats on what press.decode_to_device left on the device, added to acc_tensor (new_acc(), or any 8-byte aligned device memory of
    FILE_STATS.itemsize bytes that s5gpu_file_stats_reset_dev has reset).  Asynchronous on torch's current stream.  Returns acc_tensor."""
    import torch

    t_off = torch.from_numpy(dec.sig_off.astype(np.uint64).view(np.int64)).to(dec.dev)
    t_cap = torch.from_numpy(dec.sig_cap.astype(np.uint32).view(np.int32)).to(dec.dev)
    st = C.c_void_p(torch.cuda.current_stream(dec.dev).cuda_stream)
    check(_lib.lib().s5gpu_file_stats_accum_dev(dec.n, dec.t_sig.data_ptr(), t_off.data_ptr(), t_cap.data_ptr(), dec.t_fields.data_ptr(),
                                                acc_tensor.data_ptr(), st), "s5gpu_file_stats_accum_dev")
    torch.cuda.synchronize(dec.dev)      # t_off / t_cap die with this frame
    return acc_tensor


def to_numpy(acc_tensor):
    """the accumulator tensor as a numpy record"""
    return acc_tensor.cpu().numpy().view(FILE_STATS)[0].copy()


def _read_file(path):
    """(records, rec_method, sig_method) of a BLOW5 file, or (record lines, types line) of a SLOW5 ASCII file, told apart by the first bytes"""
    b = open(path, "rb").read()
    if b[:6] == b"BLOW5\x01":
        rec_method = {0: _lib.REC_NONE, 1: _lib.REC_ZLIB, 2: _lib.REC_ZSTD}[b[9]]
        sig_method = {0: _lib.SIG_NONE, 1: _lib.SIG_SVB_ZD, 2: _lib.SIG_EX_ZD}[b[14]]
        (hl,) = struct.unpack_from("<I", b, 64)
        off, recs = 68 + hl, []
        while not (b[off:off + 5] == b"5WOLB" and off + 5 == len(b)):
            if off + 8 > len(b):
                raise _lib.S5GpuError("%s: damaged record framing" % path)
            (sz,) = struct.unpack_from("<Q", b, off)
            if off + 8 + sz > len(b):
                raise _lib.S5GpuError("%s: damaged record framing" % path)
            recs.append(b[off + 8:off + 8 + sz])
            off += 8 + sz
        return recs, rec_method, sig_method, None
    lines = b.split(b"\n")
    types = [l for l in lines if l.startswith(b"#char*")]
    if not b.startswith(b"#slow5_version") or not types:
        raise _lib.S5GpuError("%s is neither a BLOW5 nor a SLOW5 file" % path)
    return [l for l in lines if l and l[:1] not in b"#@"], None, None, types[0]


def file_stats(path, batch=4096):
    """The accumulator of a .blow5 or .slow5 file, `batch` records per device call.  The lines of a .slow5 are converted to BLOW5 records with
    both presses none on the device first (ascii.ascii_to_blow5)."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("file_stats: batch %d" % batch)
    recs, rec_method, sig_method, types = _read_file(path)
    h = Handle()
    try:
        for lo in range(0, len(recs), batch):
            part = recs[lo:lo + batch]
            if types is not None:
                from . import ascii

                part = [r[8:] for r in ascii.ascii_to_blow5(part, ascii.aux_types(types), REC_NONE, SIG_NONE)]
                h.add(part, REC_NONE, SIG_NONE)
            else:
                h.add(part, rec_method, sig_method)
    except Exception:
        h.abandon()
        raise
    return h.close()
