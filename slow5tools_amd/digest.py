"""sum: a content digest per read, hashed on the device where the decoder left the read (include/slow5gpu.h "sum", docs/codecs.md §4.12).

The digest of a read is XXH64 (seed 0) of its CANONICAL record: the record as a BLOW5 file with record press none and signal press none stores
it, without the u64 size prefix.  It does not depend on the presses the record was stored with.  It resists accidents, not adversaries.

  record_digests : records -> digests through s5gpu_digest_stream (or s5gpu_digest_batch): compressed bytes go up, 8 bytes per read come back
  file_digests   : a .blow5 / .slow5 file -> (ids, digests, header digest) through the s5sum tool

There is no host implementation of the hash here: the library has no CPU path.
"""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from . import _lib
from . import build as _build
from ._lib import REC_ZLIB, SIG_SVB_ZD, check

S5SUM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "s5sum")


def record_digests(records, rec_method=REC_ZLIB, sig_method=SIG_SVB_ZD, raise_on_error=True, via="stream"):
    """Digests of a batch of records (bytes without the u64 prefix): a uint64 array.  A corrupt record raises; with raise_on_error=False the
    result is (digests, statuses): a corrupt record has its decode status (not 0) and digest 0, the other records' digests are valid.
    via: "stream" (the records framed in one buffer, s5gpu_digest_stream) or "batch" (one pointer per record, s5gpu_digest_batch)."""
    if via not in ("stream", "batch"):
        raise ValueError("record_digests: via must be 'stream' or 'batch'")
    L = _lib.lib()
    n = len(records)
    digests = np.zeros(n, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    if n:
        vp = C.c_void_p
        rb = [bytes(r) for r in records]
        if via == "stream":
            pos, parts, at = np.zeros(n, dtype=np.uint64), [], 0
            for i, r in enumerate(rb):
                parts.append(struct.pack("<Q", len(r)) + r)
                pos[i] = at + 8
                at += 8 + len(r)
            chunk = np.frombuffer(b"".join(parts) + bytes(64), dtype=np.uint8)
            lens = np.array([len(r) for r in rb], dtype=np.uint32)
            rc = L.s5gpu_digest_stream(n, chunk.ctypes.data_as(vp), at, pos.ctypes.data_as(vp), lens.ctypes.data_as(vp), rec_method, sig_method,
                                       digests.ctypes.data_as(vp), status.ctypes.data_as(vp))
            what = "s5gpu_digest_stream"
        else:
            rbuf = [C.create_string_buffer(r, max(len(r), 1)) for r in rb]
            rec_p = (vp * n)(*[C.addressof(b) for b in rbuf])
            rl = (C.c_size_t * n)(*[len(r) for r in rb])
            rc = L.s5gpu_digest_batch(n, rec_p, rl, rec_method, sig_method, digests.ctypes.data_as(vp), status.ctypes.data_as(vp))
            what = "s5gpu_digest_batch"
        if rc != 0 and (raise_on_error or rc != -5):
            check(rc, what)
    return digests if raise_on_error else (digests, status)


def file_digests(path, batch=4096):
    """(ids, digests, header_digest) of a .blow5 or .slow5 file, the reads in file order: ids a list of bytes, digests a uint64 array,
    header_digest an int.  Runs the s5sum tool (examples/s5sum.c), `batch` records per device call."""
    if not os.path.exists(S5SUM):
        _build.build()
    p = subprocess.run([S5SUM, "-K", str(int(batch)), os.fspath(path)], capture_output=True)
    if p.returncode != 0:
        raise _lib.S5GpuError("s5sum %s failed (exit %d): %s" % (path, p.returncode, p.stderr.decode(errors="replace").strip()))
    lines = p.stdout.split(b"\n")
    head = lines[0].split(b"\t")
    if len(head) != 4 or head[:3] != [b"#s5sum", b"1", b"xxh64"]:
        raise _lib.S5GpuError("s5sum %s: unexpected first line %r" % (path, lines[0]))
    ids, digs = [], []
    for ln in lines[1:]:
        if not ln or ln.startswith(b"#total\t"):
            break
        d, rid = ln.split(b"\t", 1)
        ids.append(rid)
        digs.append(int(d, 16))
    return ids, np.array(digs, dtype=np.uint64), int(head[3], 16)
