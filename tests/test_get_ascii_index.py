"""The read-id index of a SLOW5 file (slow5_idx_create / _load / _load_with, slow5_get_rids, slow5_get_mem), host C only.

An entry is one record line: offset = its first byte, size = its length with the newline.  The reference's expected index pins the bytes;
the edge cases are this project's choices (docs/codecs.md §4.10)."""
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess

import pytest

from slow5tools_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GA = os.path.join(HERE, "golden", "get_ascii")
MULTI = os.path.join(HERE, "golden", "example_multi_rg_v0.1.0.slow5")
MULTI_IDX = open(os.path.join(GA, "example_multi_rg_v0.1.0.slow5.idx.exp"), "rb").read()
libc = C.CDLL(None)
libc.free.argtypes = [C.c_void_p]


@pytest.fixture(scope="module")
def L():
    lib, vp = _lib.lib(), C.c_void_p
    lib.slow5_open.restype = vp
    lib.slow5_open.argtypes = [C.c_char_p, C.c_char_p]
    for f in (lib.slow5_close, lib.slow5_idx_create, lib.slow5_idx_load):
        f.argtypes = [vp]
    lib.slow5_idx_load_with.argtypes = [vp, C.c_char_p]
    lib.slow5_get_rids.restype = C.POINTER(C.c_char_p)
    lib.slow5_get_rids.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.slow5_get_mem.restype = vp
    lib.slow5_get_mem.argtypes = [C.c_char_p, C.POINTER(C.c_size_t), vp]
    lib.slow5_set_log_level.argtypes = [C.c_int]
    return lib


def parse_idx(b):
    """index bytes -> [(id, offset, size)]"""
    assert b[:9] == b"SLOW5IDX\x01" and b[-8:] == b"XDI5WOLS"
    ents, p = [], 64
    while p < len(b) - 8:
        (l,) = struct.unpack_from("<H", b, p)
        ents.append((b[p + 2:p + 2 + l],) + struct.unpack_from("<QQ", b, p + 2 + l))
        p += 2 + l + 16
    assert p == len(b) - 8
    return ents


def record_lines(data):
    """(offset, line with its line end) of every record line"""
    out, p = [], 0
    for ln in data.splitlines(keepends=True):
        if ln[:1] not in (b"#", b"@"):
            out.append((p, ln))
        p += len(ln)
    return out


def write(tmp_path, data, name="f.slow5"):
    src = str(tmp_path / name)
    open(src, "wb").write(data)
    return src


def make_index(L, path):
    f = L.slow5_open(path.encode(), b"r")
    assert f
    rc = L.slow5_idx_create(f)
    L.slow5_close(f)
    return rc


def check_lines(L, path, data, index=None):
    """the index's entries are the record lines; slow5_get_rids and slow5_get_mem (line without its line end, NUL behind it) on every id"""
    lines = record_lines(data)
    ids = [ln.split(b"\t", 1)[0] for _, ln in lines]
    f = L.slow5_open(path.encode(), b"r")
    assert f and (L.slow5_idx_load(f) if index is None else L.slow5_idx_load_with(f, index.encode())) == 0
    assert parse_idx(open(index or path + ".idx", "rb").read()) == [(i, p, len(ln)) for i, (p, ln) in zip(ids, lines)]
    n = C.c_uint64()
    rids = L.slow5_get_rids(f, C.byref(n))
    assert [rids[i] for i in range(n.value)] == ids
    for rid, (_, ln) in zip(ids, lines):
        nb = C.c_size_t()
        m = L.slow5_get_mem(rid, C.byref(nb), f)
        assert m and C.string_at(m, nb.value + 1) == ln.rstrip(b"\n").rstrip(b"\r") + b"\0"
        libc.free(m)
    L.slow5_close(f)


def test_index_of_the_reference_slow5_is_the_reference_index(L, tmp_path):
    src = write(tmp_path, open(MULTI, "rb").read())
    assert make_index(L, src) == 0
    assert open(src + ".idx", "rb").read() == MULTI_IDX
    ents = parse_idx(MULTI_IDX)
    assert len(ents) == 7 and ents[0] == (b"9ed48863-0ab8-4f05-8fbc-1ecf6e3735d6", 3631, 16452)
    check_lines(L, src, open(src, "rb").read())


def test_index_of_example2_is_the_reference_index(L, tmp_path):
    src = write(tmp_path, gzip.decompress(open(os.path.join(GA, "example2.slow5.gz"), "rb").read()))
    assert make_index(L, src) == 0
    assert open(src + ".idx", "rb").read() == open(os.path.join(GA, "example2.slow5.idx"), "rb").read()


def test_load_makes_a_missing_index_and_load_with_reads_or_makes_one_elsewhere(L, tmp_path):
    data = open(MULTI, "rb").read()
    src = write(tmp_path, data)
    other = str(tmp_path / "elsewhere.idx")
    open(other, "wb").write(MULTI_IDX)
    check_lines(L, src, data, index=other)
    assert not os.path.exists(src + ".idx")                     # the default path is left alone
    check_lines(L, src, data, index=str(tmp_path / "made.idx"))
    assert open(str(tmp_path / "made.idx"), "rb").read() == MULTI_IDX
    check_lines(L, src, data)                                    # slow5_idx_load builds <file>.idx
    assert open(src + ".idx", "rb").read() == MULTI_IDX


@pytest.mark.parametrize("kb", ["1", "20"])
def test_chunks_smaller_than_a_line(L, tmp_path, monkeypatch, kb):
    src = write(tmp_path, open(MULTI, "rb").read())
    monkeypatch.setenv("SLOW5_IDX_CHUNK_KB", kb)                 # lines are 16 .. 194 KB: cut by the chunk's end, or longer than it
    assert make_index(L, src) == 0
    assert open(src + ".idx", "rb").read() == MULTI_IDX


def test_last_line_without_a_newline_is_indexed_with_the_bytes_it_has(L, tmp_path):
    data = open(MULTI, "rb").read()[:-1]
    src = write(tmp_path, data)
    assert make_index(L, src) == 0
    full = parse_idx(MULTI_IDX)
    assert parse_idx(open(src + ".idx", "rb").read()) == full[:-1] + [full[-1][:2] + (full[-1][2] - 1,)]
    check_lines(L, src, data)


def test_crlf_line_ends_belong_to_their_line(L, tmp_path):
    data = open(MULTI, "rb").read().replace(b"\n", b"\r\n")
    src = write(tmp_path, data)
    assert make_index(L, src) == 0
    assert all(ln.endswith(b"\r\n") for _, ln in record_lines(data))
    check_lines(L, src, data)                                    # sizes count both bytes, slow5_get_mem strips both


@pytest.mark.parametrize("bad", [b"no tab at all\n", b"\n", b"\tan empty id\n"])
def test_a_record_line_without_an_id_fails_the_index(L, tmp_path, bad):
    data = open(MULTI, "rb").read()
    at = record_lines(data)[2][0]
    src = write(tmp_path, data[:at] + bad + data[at:])
    L.slow5_set_log_level(0)
    try:
        assert make_index(L, src) == -1
    finally:
        L.slow5_set_log_level(3)
    assert not os.path.exists(src + ".idx")


def test_s5view_index_writes_the_slow5_index(tmp_path):
    src = write(tmp_path, open(MULTI, "rb").read())
    subprocess.run([os.path.join(os.path.dirname(HERE), "slow5tools_amd", "s5view"), "--index", src], check=True, timeout=120)
    assert open(src + ".idx", "rb").read() == MULTI_IDX
