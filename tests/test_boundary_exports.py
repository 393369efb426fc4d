"""SURVEY 8(b) symbols added in round 2, each driven through the C ABI the way its slow5tools call site uses it:
  slow5_rec_fwrite         /root/reference/src/get.c:89, src/read_fast5.c:177
  slow5_decode             /root/reference/src/skim.c:320
  slow5_get_next_bytes     /root/reference/src/skim.c:385
  slow5_open_with          /root/reference/src/view.c:192, src/degrade.c:423
  slow5_set_log_level / slow5_set_exit_condition   /root/reference/src/main.c:246-247
  slow5_set_skip_rid       /root/reference/src/get.c:194
  slow5_ptr_compress / slow5_ptr_depress           (stateful press API, SURVEY 8b last row) incl. ex-zd solo stages
and the slow5lib-type-free hooks of include/slow5gpu_hooks.h."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from blow5_fixture import Blow5, golden, read_slow5_ascii
from test_compat_api import File, InnerPress, Press, PressMethod, Rec, _malloc_copy, libc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NONE, ZLIB, SVB, ZSTD, EXZD = 0, 1, 2, 3, 4
ASCII, BINARY = 1, 2


class GpuRead(C.Structure):
    _fields_ = [("read_id", C.c_void_p), ("read_id_len", C.c_uint16), ("read_group", C.c_uint32),
                ("digitisation", C.c_double), ("offset", C.c_double), ("range", C.c_double), ("sampling_rate", C.c_double),
                ("len_raw_signal", C.c_uint64), ("raw_signal", C.c_void_p), ("aux", C.c_void_p), ("aux_len", C.c_uint64)]


@pytest.fixture(scope="module")
def L():
    from slow5tools_amd import _lib

    lib = _lib.lib()
    _lib.check(lib.s5gpu_init(0), "s5gpu_init")
    vp, sz = C.c_void_p, C.c_size_t
    lib.slow5_press_init.restype = C.POINTER(Press)
    lib.slow5_press_init.argtypes = [PressMethod]
    lib.slow5_press_free.argtypes = [C.POINTER(Press)]
    lib.slow5_open.restype = C.POINTER(File)
    lib.slow5_open.argtypes = [C.c_char_p, C.c_char_p]
    lib.slow5_open_with.restype = C.POINTER(File)
    lib.slow5_open_with.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.slow5_close.argtypes = [C.POINTER(File)]
    lib.slow5_get_next_bytes.argtypes = [C.POINTER(vp), C.POINTER(sz), C.POINTER(File)]
    lib.slow5_decode.argtypes = [C.POINTER(vp), C.POINTER(sz), C.POINTER(C.POINTER(Rec)), C.POINTER(File)]
    lib.slow5_rec_fwrite.argtypes = [vp, C.POINTER(Rec), vp, C.c_int, C.POINTER(Press)]
    lib.slow5_rec_free.argtypes = [C.POINTER(Rec)]
    lib.slow5_ptr_compress.restype = vp
    lib.slow5_ptr_compress.argtypes = [C.POINTER(InnerPress), vp, sz, C.POINTER(sz)]
    lib.slow5_ptr_depress.restype = vp
    lib.slow5_ptr_depress.argtypes = [C.POINTER(InnerPress), vp, sz, C.POINTER(sz)]
    lib.slow5_ptr_compress_solo.restype = vp
    lib.slow5_ptr_compress_solo.argtypes = [C.c_int, vp, sz, C.POINTER(sz)]
    lib.slow5_ptr_depress_solo.restype = vp
    lib.slow5_ptr_depress_solo.argtypes = [C.c_int, vp, sz, C.POINTER(sz)]
    lib.slow5_set_log_level.argtypes = [C.c_int]
    lib.slow5_set_exit_condition.argtypes = [C.c_int]
    lib.slow5_idx_load.argtypes = [C.POINTER(File)]
    lib.slow5_get.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Rec)), C.POINTER(File)]
    lib.slow5_gpu_hook_error.restype = C.c_char_p
    lib.slow5_gpu_hook_recompress.argtypes = [C.c_int64, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.slow5_gpu_hook_convert.argtypes = [C.c_int64, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, vp, C.c_int,
                                           C.POINTER(vp), C.POINTER(sz)]
    lib.slow5_gpu_hook_depress_parse.argtypes = [C.c_int64, C.POINTER(vp), C.POINTER(sz), C.c_int, C.c_int, C.POINTER(GpuRead)]
    lib.slow5_gpu_hook_rec_to_mem.argtypes = [C.c_int64, C.POINTER(GpuRead), C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.slow5_set_log_level(0)     # the negative cases below would otherwise print their error lines
    return lib


libc.fopen.restype = C.c_void_p
libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
libc.fclose.argtypes = [C.c_void_p]


def test_get_next_bytes_and_decode_walk_a_file_like_skim(L):
    """src/skim.c:385 + :320 — slow5_get_next_bytes until SLOW5_ERR_EOF (-1), slow5_decode each record"""
    path = golden("sp1_dna.blow5")
    want = Blow5(path)
    f = L.slow5_open_with(path.encode(), b"r", BINARY)
    assert f
    sigs = []
    for i in range(len(want.records) + 1):
        mem, nb = C.c_void_p(), C.c_size_t()
        ret = L.slow5_get_next_bytes(C.byref(mem), C.byref(nb), f)
        if i == len(want.records):
            assert ret == -1                                    # SLOW5_ERR_EOF
            break
        assert ret == 0 and C.string_at(mem, nb.value) == want.records[i]
        rec = C.POINTER(Rec)()
        assert L.slow5_decode(C.byref(mem), C.byref(nb), C.byref(rec), f) == 0
        libc.free(mem)                                          # src/skim.c:323: the caller frees the record
        r = rec.contents
        pay = zlib.decompress(want.records[i])
        idl = struct.unpack_from("<H", pay, 0)[0]
        assert C.string_at(r.read_id, r.read_id_len) == pay[2:2 + idl]
        sigs.append(np.frombuffer(C.string_at(r.raw_signal, 2 * r.len_raw_signal), dtype=np.int16).copy())
        L.slow5_rec_free(rec)
    L.slow5_close(f)
    assert len(sigs) == len(want.records) and sum(s.size for s in sigs) == 23659
    # a corrupt record: slow5_decode < 0
    f = L.slow5_open(path.encode(), b"r")
    bad = bytearray(want.records[0]); bad[30] ^= 0xFF
    mem, nb = C.c_void_p(_malloc_copy(bytes(bad))), C.c_size_t(len(bad))
    rec = C.POINTER(Rec)()
    assert L.slow5_decode(C.byref(mem), C.byref(nb), C.byref(rec), f) < 0
    libc.free(mem)
    L.slow5_close(f)


def test_open_with_checks_the_named_format(L):
    b5, s5 = golden("exp_1_lossless.blow5"), golden("exp_1_lossless.slow5")
    for path, fmt in ((b5, BINARY), (s5, ASCII), (b5, 0), (s5, 0)):
        f = L.slow5_open_with(path.encode(), b"r", fmt)
        assert f and f.contents.format == (BINARY if path == b5 else ASCII)
        L.slow5_close(f)
    assert not L.slow5_open_with(b5.encode(), b"r", ASCII)      # --from slow5 on a BLOW5 file
    assert not L.slow5_open_with(s5.encode(), b"r", BINARY)
    assert not L.slow5_open_with(b5.encode(), b"r", 9)
    assert not L.slow5_open_with(b"/nonexistent.blow5", b"r", BINARY)


def test_rec_fwrite_binary_and_ascii_reproduce_the_reference_files(L, tmp_path):
    """src/get.c:89 — slow5_get then slow5_rec_fwrite in the output format: BLOW5 bytes equal the golden record, the ASCII line
    equals the golden .slow5 line"""
    src = tmp_path / "exp_1_lossless_zlib_svb_v0.2.0.blow5"          # a copy: slow5_idx_load writes the missing .idx beside the file
    shutil.copy(golden(src.name), src)
    f = L.slow5_open(str(src).encode(), b"r")
    assert L.slow5_idx_load(f) == 0
    rec = C.POINTER(Rec)()
    assert L.slow5_get(b"a649a4ae-c43d-492a-b6a1-a5b8b8076be4", C.byref(rec), f) == 0
    want = Blow5(golden("exp_1_lossless.blow5"))
    aux_meta = C.cast(f.contents.header, C.POINTER(C.c_uint8 * 32))   # header->aux_meta sits behind version/num_rg/data/data_len
    # struct slow5_hdr { version[3]; u32 num_read_groups; char *data; u32 data_len; aux_meta* } -> offset 32 on LP64
    am = C.c_void_p.from_address(C.addressof(aux_meta.contents) + 24).value
    out = tmp_path / "one.blow5body"
    fp = libc.fopen(str(out).encode(), b"wb")
    none = L.slow5_press_init(PressMethod(NONE, NONE))
    n = L.slow5_rec_fwrite(fp, rec, am, BINARY, none)
    libc.fclose(fp)
    body = open(out, "rb").read()
    assert n == len(body) and body == struct.pack("<Q", len(want.records[0])) + want.records[0]
    out2 = tmp_path / "one.slow5line"
    fp = libc.fopen(str(out2).encode(), b"wb")
    n = L.slow5_rec_fwrite(fp, rec, am, ASCII, none)
    libc.fclose(fp)
    line = open(out2, "rb").read()
    gold_lines = [l for l in open(golden("exp_1_lossless.slow5"), "rb").read().split(b"\n") if l and l[:1] not in b"#@"]
    assert n == len(line) and line == gold_lines[0] + b"\n"
    assert L.slow5_rec_fwrite(None, rec, am, BINARY, none) == -1
    L.slow5_press_free(none)
    L.slow5_rec_free(rec)
    L.slow5_close(f)


def test_stateful_ptr_press_calls_and_exzd_solo(L):
    rng = np.random.default_rng(3)
    sig = (500 + 40 * rng.standard_normal(20000)).astype(np.int16)
    sig[100] = 9000; sig[101] = -3000                     # exceptions for ex-zd
    p = L.slow5_press_init(PressMethod(ZLIB, EXZD))
    n = C.c_size_t()
    q = L.slow5_ptr_compress(p.contents.signal_press, sig.ctypes.data, sig.nbytes, C.byref(n))
    blob = C.string_at(q, n.value); libc.free(q)
    assert blob == ob.exzd_encode(sig)                    # bit-exact with the oracle (pinned on the reference's ex-zd fixtures)
    q = L.slow5_ptr_depress(p.contents.signal_press, blob, len(blob), C.byref(n))
    back = np.frombuffer(C.string_at(q, n.value), dtype=np.int16); libc.free(q)
    assert np.array_equal(back, sig)
    q = L.slow5_ptr_compress(p.contents.record_press, blob, len(blob), C.byref(n))
    z = C.string_at(q, n.value); libc.free(q)
    assert zlib.decompress(z) == blob
    q = L.slow5_ptr_depress(p.contents.record_press, z, len(z), C.byref(n))
    assert C.string_at(q, n.value) == blob; libc.free(q)
    assert not L.slow5_ptr_compress(None, blob, len(blob), C.byref(n))
    # edge lengths through the ex-zd solo stages
    for m in (0, 1, 2, 4095, 4096, 4097):
        s = sig[:m].copy()
        q = L.slow5_ptr_compress_solo(EXZD, s.ctypes.data if m else None, s.nbytes, C.byref(n))
        b = C.string_at(q, n.value); libc.free(q)
        assert b == ob.exzd_encode(s), m
        q = L.slow5_ptr_depress_solo(EXZD, b, len(b), C.byref(n))
        assert np.array_equal(np.frombuffer(C.string_at(q, n.value), dtype=np.int16), s); libc.free(q)
    assert not L.slow5_ptr_depress_solo(EXZD, blob[:40], 40, C.byref(n))      # truncated blob
    L.slow5_press_free(p)


def test_skip_rid_and_exit_condition_in_a_fresh_process(tmp_path):
    """slow5_set_exit_condition(SLOW5_EXIT_ON_ERR) makes an error fatal (what main.c:247 selects); slow5_set_skip_rid keeps a
    missing read id from being one (get.c:194).  Process state, so each case runs in its own interpreter."""
    code = r'''
import ctypes as C, sys
sys.path.insert(0, %r); sys.path.insert(0, %r + "/tests")
from slow5tools_amd import _lib
from test_compat_api import File, Rec
L = _lib.lib(); _lib.check(L.s5gpu_init(0), "init")
L.slow5_open.restype = C.POINTER(File); L.slow5_open.argtypes = [C.c_char_p, C.c_char_p]
L.slow5_idx_load.argtypes = [C.POINTER(File)]; L.slow5_get.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Rec)), C.POINTER(File)]
f = L.slow5_open(%r.encode(), b"r"); assert L.slow5_idx_load(f) == 0
mode = sys.argv[1]
L.slow5_set_log_level(1)
if mode == "skip": L.slow5_set_skip_rid()
L.slow5_set_exit_condition(1)
rec = C.POINTER(Rec)()
rc = L.slow5_get(b"no-such-read", C.byref(rec), f)
print("returned", rc)
'''
    import shutil

    path = tmp_path / "x.blow5"
    shutil.copy(golden("example_multi_rg_v0.2.0.blow5"), path)
    for mode, want_rc, want_out in (("skip", 0, "returned -7"), ("strict", 1, "")):
        r = subprocess.run([sys.executable, "-c", code % (ROOT, ROOT, str(path)), mode], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == want_rc, r.stdout + r.stderr
        assert want_out in r.stdout
        if mode == "strict":
            assert "not in the index" in r.stderr and "returned" not in r.stdout      # exit(EXIT_FAILURE) inside the call


def test_hooks_without_slow5lib_types(L):
    """include/slow5gpu_hooks.h: the same workers with methods as plain ints (what a patched view.c calls beside <slow5/slow5.h>)"""
    src = Blow5(golden("merged_expected_zlib_svb.blow5"))
    n = len(src.records)
    mem = (C.c_void_p * n)(*[_malloc_copy(r) for r in src.records])
    nb = (C.c_size_t * n)(*[len(r) for r in src.records])
    out = (C.c_void_p * n)(); ol = (C.c_size_t * n)()
    assert L.slow5_gpu_hook_recompress(n, mem, nb, ZLIB, SVB, NONE, NONE, None, 0, out, ol) == 0, L.slow5_gpu_hook_error()
    assert all(not mem[i] for i in range(n))                        # inputs freed like the reference's worker does
    plain = [C.string_at(out[i], ol[i]) for i in range(n)]
    for i in range(n):
        libc.free(out[i])
        pay = zlib.decompress(src.records[i])
        idl = struct.unpack_from("<H", pay, 0)[0]
        L0 = struct.unpack_from("<Q", pay, 2 + idl + 36)[0]
        sig = ob.svbzd_decode(pay[2 + idl + 44: 2 + idl + 44 + L0])
        want = pay[:2 + idl + 36] + struct.pack("<Q", sig.size) + sig.tobytes() + pay[2 + idl + 44 + L0:]
        assert plain[i][8:] == want
    assert L.slow5_gpu_hook_recompress(1, mem, nb, 9, SVB, NONE, NONE, None, 0, out, ol) == -1
    # depress_parse -> rec_to_mem with the hook's own read struct
    mem = (C.c_void_p * n)(*[_malloc_copy(r) for r in src.records])
    nb = (C.c_size_t * n)(*[len(r) for r in src.records])
    reads = (GpuRead * n)()
    assert L.slow5_gpu_hook_depress_parse(n, mem, nb, ZLIB, SVB, reads) == 0
    for i in range(n):
        pay = zlib.decompress(src.records[i])
        assert C.string_at(mem[i], nb[i]) == pay                     # *mem now holds the uncompressed record
        idl = struct.unpack_from("<H", pay, 0)[0]
        assert C.string_at(reads[i].read_id, reads[i].read_id_len) == pay[2:2 + idl]
        assert reads[i].aux_len == 0 or C.string_at(reads[i].aux, reads[i].aux_len) == pay[len(pay) - reads[i].aux_len:]
    assert L.slow5_gpu_hook_rec_to_mem(n, reads, 0, ZLIB, SVB, out, ol) == 0
    for i in range(n):
        got = C.string_at(out[i], ol[i]); libc.free(out[i])
        assert zlib.decompress(got[8:]) == zlib.decompress(src.records[i])
        libc.free(reads[i].raw_signal); libc.free(mem[i])
    # ASCII in, BLOW5 out through the convert hook with the header's types line
    lines = [l for l in open(golden("exp_1_lossless.slow5"), "rb").read().split(b"\n") if l and l[:1] not in b"#@"]
    types_line = [l for l in open(golden("exp_1_lossless.slow5"), "rb").read().split(b"\n") if l.startswith(b"#char*")][0]
    m1 = (C.c_void_p * 1)(_malloc_copy(lines[0])); n1 = (C.c_size_t * 1)(len(lines[0]))
    o1 = (C.c_void_p * 1)(); l1 = (C.c_size_t * 1)()
    assert L.slow5_gpu_hook_convert(1, m1, n1, ASCII, NONE, NONE, types_line, BINARY, NONE, NONE, None, 0, o1, l1) == 0
    want = Blow5(golden("exp_1_lossless.blow5")).records[0]
    assert C.string_at(o1[0], l1[0]) == struct.pack("<Q", len(want)) + want
    libc.free(o1[0])
