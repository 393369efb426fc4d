"""SLOW5 -> SLOW5 on the device (s5gpu_ascii_to_ascii_stream / _batch), slow5_get on a .slow5, and s5get in the shape of slow5tools get.

The stream call must print every line as slow5_gpu_convert_batch(ASCII -> ASCII) does, and set a bad line's status as ascii_to_blow5 does.
s5get runs the 11 cases of the reference's test/test_get.sh on its example2.slow5 (committed gzip'd, as the expected SLOW5 outputs are)."""
import ctypes as C
import glob
import gzip
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from blow5_fixture import Blow5
from slow5tools_amd import _lib, ascii

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GA = os.path.join(GOLDEN, "get_ascii")
S5GET, S5VIEW = (os.path.join(os.path.dirname(HERE), "slow5tools_amd", x) for x in ("s5get", "s5view"))
ASCII, ERR_NOMEM, ERR_DATA = 1, -3, -5
SLOW5_FILES = sorted(os.path.relpath(p, GOLDEN) for p in glob.glob(os.path.join(GOLDEN, "**", "*.slow5"), recursive=True))

pytestmark = pytest.mark.gpu


class PressMethod(C.Structure):
    _fields_ = [("record_method", C.c_int), ("signal_method", C.c_int)]


class AuxMeta(C.Structure):
    _fields_ = [("num", C.c_uint32), ("types", C.c_void_p)]


libc = C.CDLL(None)
libc.malloc.restype = C.c_void_p
libc.malloc.argtypes = [C.c_size_t]
libc.free.argtypes = [C.c_void_p]


@pytest.fixture(scope="module")
def L():
    lib, vp = _lib.lib(), C.c_void_p
    _lib.check(lib.s5gpu_init(0), "s5gpu_init")
    lib.slow5_gpu_convert_batch.argtypes = [C.c_int64, vp, vp, C.c_int, PressMethod, C.POINTER(AuxMeta), C.c_int, PressMethod, vp, C.c_int, vp, vp]
    lib.slow5_open.restype = vp
    lib.slow5_open.argtypes = [C.c_char_p, C.c_char_p]
    lib.slow5_close.argtypes = [vp]
    lib.slow5_idx_load.argtypes = [vp]
    return lib


def gz(name):
    return gzip.decompress(open(os.path.join(GA, name + ".gz"), "rb").read())


def split_slow5(data):
    """(header bytes, aux type codes, record lines with their newline)"""
    lines = data.splitlines(keepends=True)
    k = next(i for i, ln in enumerate(lines) if ln.startswith(b"#read_id"))
    return b"".join(lines[:k + 1]), ascii.aux_types(lines[k - 1]), [ln for ln in lines[k + 1:] if ln.strip()]


def ids_of(lines):
    return [ln.split(b"\t", 1)[0] for ln in lines]


def convert(L, lines, types, new_rg=None, drop_aux=False):
    """the two-call route: slow5_gpu_convert_batch(ASCII -> ASCII)"""
    n = len(lines)
    mem = (C.c_void_p * n)(*[libc.malloc(max(len(ln), 1)) for ln in lines])
    for i, ln in enumerate(lines):
        C.memmove(mem[i], ln, len(ln))
    tb = (C.c_uint8 * max(len(types), 1))(*types)
    am = AuxMeta(len(types), C.cast(tb, C.c_void_p))
    rg = None if new_rg is None else np.ascontiguousarray(new_rg, dtype=np.uint32)
    out, out_len, none = (C.c_void_p * n)(), (C.c_size_t * n)(), PressMethod(0, 0)
    assert L.slow5_gpu_convert_batch(n, mem, (C.c_size_t * n)(*map(len, lines)), ASCII, none, C.byref(am) if types else None, ASCII, none,
                                     None if rg is None else rg.ctypes.data, int(drop_aux), out, out_len) == 0
    res = [C.string_at(out[i], out_len[i]) for i in range(n)]
    for p in out:
        libc.free(p)
    return res


def stream(L, lines, types, new_rg=None, drop_aux=False, cap=None):
    """s5gpu_ascii_to_ascii_stream on the lines back to back in one chunk (32 bytes behind) -> (rc, block, out_off, status)"""
    n = len(lines)
    ln_len = np.array([len(x) for x in lines], dtype=np.uint32)
    pos = np.concatenate([[0], np.cumsum(ln_len, dtype=np.uint64)[:-1]]).astype(np.uint64)
    at = int(ln_len.sum())
    chunk = C.create_string_buffer(b"".join(lines) + b"\0" * 32, at + 32)
    tb = (C.c_uint8 * max(len(types), 1))(*types)
    rg = None if new_rg is None else np.ascontiguousarray(new_rg, dtype=np.uint32)
    cap = at * 2 + 4096 if cap is None else cap
    out, off, st = C.create_string_buffer(cap), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    rc = L.s5gpu_ascii_to_ascii_stream(n, chunk, at, pos.ctypes.data, ln_len.ctypes.data, len(types), tb, None if rg is None else rg.ctypes.data,
                                       int(drop_aux), out, cap, off.ctypes.data, st.ctypes.data)
    return rc, out.raw[:int(off[n])] if rc == 0 else None, off, st


@pytest.mark.parametrize("rel", SLOW5_FILES)
def test_stream_and_batch_equal_the_convert_route_on_every_committed_slow5(L, rel):
    _, types, lines = split_slow5(open(os.path.join(GOLDEN, rel), "rb").read())
    want = convert(L, lines, types)
    rc, block, off, st = stream(L, lines, types)
    assert rc == 0 and not st.any() and block == b"".join(want)
    assert np.diff(off).tolist() == [len(w) for w in want]
    assert ascii.ascii_to_ascii(lines, types) == want
    assert ascii.ascii_to_ascii([ln.rstrip(b"\n") for ln in lines], types) == want     # lines without their newline


@pytest.mark.parametrize("rel", ["example_multi_rg_v0.1.0.slow5", "aux_array_exp_lossless.slow5", "merge_rg1.slow5"])
def test_new_read_group_and_drop_aux(L, rel):
    _, types, lines = split_slow5(open(os.path.join(GOLDEN, rel), "rb").read())
    rg = np.arange(len(lines), dtype=np.uint32) * 7 + 3
    for kw in (dict(new_rg=rg), dict(drop_aux=True), dict(new_rg=rg, drop_aux=True)):
        want = convert(L, lines, types, **kw)
        rc, block, _, _ = stream(L, lines, types, **kw)
        assert rc == 0 and block == b"".join(want), kw
        assert ascii.ascii_to_ascii(lines, types, new_read_group=kw.get("new_rg"), drop_aux=kw.get("drop_aux", False)) == want
        assert not kw.get("drop_aux") or all(w.count(b"\t") == 7 for w in want)


def test_too_small_a_buffer_reports_the_room_needed(L):
    _, types, lines = split_slow5(open(os.path.join(GOLDEN, "example_multi_rg_v0.1.0.slow5"), "rb").read())
    want = b"".join(convert(L, lines, types))
    rc, _, off, _ = stream(L, lines, types, cap=1000)
    assert rc == ERR_NOMEM and int(off[0]) == len(want)
    assert stream(L, lines, types, cap=int(off[0]))[:2] == (0, want)


def test_bad_lines_get_the_statuses_of_ascii_to_blow5(L):
    _, types, lines = split_slow5(open(os.path.join(GOLDEN, "exp_1_lossless.slow5"), "rb").read())
    f = lines[0].rstrip(b"\n").split(b"\t")
    sig = f[7].split(b",")

    def with_sig(s, n=None):
        return b"\t".join(f[:6] + [str(len(s) if n is None else n).encode(), b",".join(s)] + f[8:]) + b"\n"

    # host parse 16, bad character 1, out of int16 2, empty sample 3, count mismatch 4
    for bad in (b"only\tthree\tcolumns\n", with_sig([b"12a"] + sig[1:]), with_sig([b"40000"] + sig[1:]), with_sig([b""] + sig[1:]),
                with_sig(sig, n=len(sig) + 1)):
        batch, st_b, st_a = [lines[0], bad, lines[0]], [0] * 3, [0] * 3
        with pytest.raises(_lib.S5GpuError):
            ascii.ascii_to_blow5(batch, types, rec_method=0, sig_method=0, status=st_b)
        with pytest.raises(_lib.S5GpuError):
            ascii.ascii_to_ascii(batch, types, status=st_a)
        rc, _, _, st = stream(L, batch, types)
        assert rc == ERR_DATA and st_b[1] != 0 and list(st) == st_b == st_a, bad[:40]


def test_slow5_get_on_a_slow5_file_gives_the_read_of_its_blow5_twin(L, tmp_path):
    from test_compat_api import Rec

    L.slow5_get.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Rec)), C.c_void_p]
    L.slow5_rec_free.argtypes = [C.POINTER(Rec)]
    got = []
    for name in ("example_multi_rg_v0.1.0.slow5", "example_multi_rg_v0.1.0.blow5"):
        shutil.copy(os.path.join(GOLDEN, name), tmp_path / name)
        f = L.slow5_open(str(tmp_path / name).encode(), b"r")
        assert f and L.slow5_idx_load(f) == 0
        reads = []
        for rid in (b"9ed48863-0ab8-4f05-8fbc-1ecf6e3735d6", b"ddbe1302-2998-4def-9ccc-c3b572c50574", b"d2f5aad8-86fb-4be2-9be3-0cac85ed4eef"):
            rec = C.POINTER(Rec)()
            assert L.slow5_get(rid, C.byref(rec), f) == 0
            r = rec.contents
            reads.append((C.string_at(r.read_id, r.read_id_len), r.read_group, C.string_at(r.raw_signal, 2 * r.len_raw_signal)))
            L.slow5_rec_free(rec)
        L.slow5_close(f)
        got.append(reads)
    assert got[0] == got[1]


# ---- s5get: the reference's test/test_get.sh ----
@pytest.fixture(scope="module")
def ex2(tmp_path_factory):
    d = tmp_path_factory.mktemp("get")
    (d / "example2.slow5").write_bytes(gz("example2.slow5"))
    for name in ("list.txt", "list_weird_newline.txt", "list_windows.txt", "list_with_invalid_reads.txt"):
        shutil.copy(os.path.join(GA, name), d / name)
    (d / "custom").mkdir()
    shutil.copy(os.path.join(GA, "example2.slow5.idx"), d / "custom" / "example2.slow5.idx")
    return d


def s5get(*args, stdin=None):
    return subprocess.run([S5GET] + [str(a) for a in args], capture_output=True, input=stdin, timeout=300)


@pytest.mark.parametrize("case,args,exp", [
    (1, ["r1", "--to", "slow5"], "expected_extracted_reads.slow5"),
    (2, ["r1", "r5", "r3", "--to", "slow5"], "expected_extracted_reads2.slow5"),
    (3, ["--list", "{d}/list.txt", "--to", "slow5"], "expected_extracted_reads3.slow5"),
    (4, ["-t", "2", "r1", "r5", "r3", "--to", "slow5"], "expected_extracted_reads2.slow5"),
    (10, ["--list", "{d}/list_weird_newline.txt", "--to", "slow5"], "expected_extracted_reads3.slow5"),
    (11, ["--list", "{d}/list_windows.txt", "--to", "slow5"], "expected_extracted_reads3.slow5"),
])
def test_get_cases_with_slow5_output(ex2, case, args, exp):
    r = s5get(ex2 / "example2.slow5", *[a.format(d=ex2) for a in args])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == gz(exp), "testcase %d" % case


@pytest.mark.parametrize("case", [5, 6, 9])
def test_get_cases_with_blow5_output(ex2, tmp_path, case):
    """GPU deflate is not zlib's: header bytes identical, the same records in order inflating to the expected payloads, the EOF marker"""
    out, ids, press = tmp_path / "extracted_reads2.blow5", ["r1", "r5", "r3"], ["-c", "zlib", "-s", "none"]
    extra = {5: ["--to", "blow5"], 6: ["-o", out], 9: ["--index", ex2 / "custom" / "example2.slow5.idx", "--to", "blow5"]}[case]
    r = s5get(ex2 / "example2.slow5", *(ids + extra + press))
    assert r.returncode == 0, r.stderr.decode()
    if case != 6:
        out.write_bytes(r.stdout)
    got, want = Blow5(str(out)), Blow5(os.path.join(GOLDEN, "ref", "exp", "get", "expected_extracted_reads.blow5"))
    assert got.raw[:68 + len(want.header_text)] == want.raw[:68 + len(want.header_text)]
    assert [zlib.decompress(x) for x in got.records] == [zlib.decompress(x) for x in want.records]   # (Blow5 stops at the EOF marker)


def test_get_cases_7_and_8_missing_ids(ex2):
    assert s5get(ex2 / "example2.slow5", "--list", ex2 / "list_with_invalid_reads.txt", "--to", "slow5").returncode != 0
    r = s5get(ex2 / "example2.slow5", "--skip", "--list", ex2 / "list_with_invalid_reads.txt", "--to", "slow5")
    assert r.returncode == 0, r.stderr.decode()
    head, _, lines = split_slow5(r.stdout)
    whead, _, wlines = split_slow5(gz("expected_extracted_reads3.slow5"))                        # r1 r3 r4
    assert head == whead and lines == [wlines[1], wlines[2], wlines[0]]                            # list: r100 r3 r500 r4 r1 r600
    assert b"r100" in r.stderr and b"r600" in r.stderr


def test_ids_on_stdin_and_small_batches(ex2):
    r = s5get(ex2 / "example2.slow5", "--to", "slow5", "-K", "1", stdin=b"r1\nr3\n\nr4\r\n")
    assert r.returncode == 0 and r.stdout == gz("expected_extracted_reads3.slow5"), r.stderr.decode()


def test_blow5_input_to_slow5_equals_s5view_restricted_to_the_ids(tmp_path):
    src, full = tmp_path / "in.blow5", tmp_path / "full.slow5"
    shutil.copy(os.path.join(GOLDEN, "example_multi_rg_v0.1.0.blow5"), src)
    r = subprocess.run([S5VIEW, str(src), str(full)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    head, _, lines = split_slow5(full.read_bytes())
    ids = ids_of(lines)[::-1][:5] + ids_of(lines)[:1]
    r = s5get(src, "--to", "slow5", *[i.decode() for i in ids])
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == head + b"".join(dict(zip(ids_of(lines), lines))[i] for i in ids)
    # the .slow5 twin (its header text differs from the BLOW5's): the same reads in order; -o and --index elsewhere
    r = s5get(os.path.join(GOLDEN, "example_multi_rg_v0.1.0.slow5"), "-o", tmp_path / "x.slow5", "--index", tmp_path / "x.idx", *[i.decode() for i in ids])
    assert r.returncode == 0, r.stderr.decode()
    assert ids_of(split_slow5((tmp_path / "x.slow5").read_bytes())[2]) == ids and (tmp_path / "x.idx").exists()


def test_legacy_positional_form_gives_the_same_bytes(tmp_path):
    src = tmp_path / "in.blow5"
    shutil.copy(os.path.join(GOLDEN, "example_multi_rg_v0.2.0.blow5"), src)
    ids = [zlib.decompress(x)[2:38] for x in Blow5(str(src)).records][::-1]
    (tmp_path / "ids.txt").write_bytes(b"\n".join(ids) + b"\n")
    legacy, new = tmp_path / "legacy.blow5", tmp_path / "new.blow5"
    assert subprocess.run([S5GET, str(src), str(tmp_path / "ids.txt"), str(legacy), "zlib", "svb-zd"], timeout=300).returncode == 0
    assert s5get(src, "-l", tmp_path / "ids.txt", "-o", new, "-c", "zlib", "-s", "svb-zd").returncode == 0
    assert new.read_bytes() == legacy.read_bytes()
    assert [zlib.decompress(x)[2:38] for x in Blow5(str(new)).records] == ids
