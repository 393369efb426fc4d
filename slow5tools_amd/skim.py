"""slow5tools skim on the GPU (include/slow5gpu.h: s5gpu_skim_layout_parse, s5gpu_skim_stream; docs/codecs.md §4.9).

skim_records(records, header_text, rec_method, sig_method) -> list of lines (bytes, each ending in b"\\n"), one per record
skim_file(path) -> the whole output of `s5skim path`: the column line, then one line per record
Records are BLOW5 record bytes without their u64 size prefix; methods are the library's codes (_lib.REC_*, _lib.SIG_*).
"""
import ctypes as C
import struct

import numpy as np

from . import _lib

COLUMNS = b"#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal"


class SkimError(_lib.S5GpuError):
    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


def layout(header_text):
    """the header's skim layout (s5gpu_skim_layout_t); SkimError when skim cannot read it"""
    lay = _lib.SkimLayout()
    h = bytes(header_text)
    rc = _lib.lib().s5gpu_skim_layout_parse(h, len(h), C.byref(lay))
    if rc != 0:
        raise SkimError("s5gpu_skim_layout_parse failed (rc=%d): %s" % (rc, _lib.lib().s5gpu_last_error().decode(errors="replace")))
    return lay


def aux_names(lay):
    return [bytes(lay.text[lay.name_off[a] : lay.name_off[a] + lay.name_len[a]]) for a in range(lay.n_aux)]


def skim_records(records, header_text, rec_method, sig_method, out_cap=None):
    """one skim line per record, formatted on the GPU"""
    lay = header_text if isinstance(header_text, _lib.SkimLayout) else layout(header_text)
    n = len(records)
    if n == 0:
        return []
    pos = np.zeros(n, dtype=np.uint64)
    lens = np.array([len(r) for r in records], dtype=np.uint32)
    at = 0
    for i, r in enumerate(records):
        pos[i] = at
        at += (len(r) + 15) // 16 * 16
    chunk = np.zeros(at + 16, dtype=np.uint8)
    for i, r in enumerate(records):
        chunk[int(pos[i]) : int(pos[i]) + len(r)] = np.frombuffer(r, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.int32)
    cap = out_cap if out_cap is not None else 192 * n + 4096
    L = _lib.lib()
    for _ in range(2):
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        rc = L.s5gpu_skim_stream(n, chunk.ctypes.data, at, pos.ctypes.data, lens.ctypes.data, rec_method, sig_method, C.byref(lay),
                                 out.ctypes.data, cap, off.ctypes.data, status.ctypes.data)
        if rc == -3 and out_cap is None:   # S5GPU_ERR_NOMEM: off[0] = the room needed
            cap = int(off[0])
            continue
        break
    if rc != 0:
        raise SkimError("s5gpu_skim_stream failed (rc=%d): %s" % (rc, L.s5gpu_last_error().decode(errors="replace")), status)
    text = out.tobytes()
    return [text[int(off[i]) : int(off[i + 1])] for i in range(n)]


def _read_blow5(path):
    b = open(path, "rb").read()
    if b[:6] != b"BLOW5\x01":
        raise SkimError("%s is not a BLOW5 file" % path)
    rec_method = {0: _lib.REC_NONE, 1: _lib.REC_ZLIB, 2: _lib.REC_ZSTD}[b[9]]
    sig_method = {0: _lib.SIG_NONE, 1: _lib.SIG_SVB_ZD, 2: _lib.SIG_EX_ZD}[b[14]]
    (hl,) = struct.unpack_from("<I", b, 64)
    header = b[68 : 68 + hl]
    off, recs = 68 + hl, []
    while not (b[off : off + 5] == b"5WOLB" and off + 5 == len(b)):
        (sz,) = struct.unpack_from("<Q", b, off)
        recs.append(b[off + 8 : off + 8 + sz])
        off += 8 + sz
    return header, recs, rec_method, sig_method


def skim_file(path):
    """what `s5skim path` prints: the column line and every record's line"""
    header, recs, rec_method, sig_method = _read_blow5(path)
    lay = layout(header)
    head = COLUMNS + b"".join(b"\t" + nm for nm in aux_names(lay)) + b"\n"
    return head + b"".join(skim_records(recs, lay, rec_method, sig_method))
