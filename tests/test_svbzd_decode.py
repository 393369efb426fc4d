"""svb-zd decoders on hand-made blobs: every device route against a plain numpy reference, valid and malformed.

The encoders (ours and slow5lib's) only ever write codes 0-2 at minimal width into well-formed blobs.  The format allows more:
code-3 (4-byte) values, widths wider than needed, sums that wrap int16 and int32 — and a decoder has to reject a blob whose count,
key area or data area does not add up (status 7, as the CPU decoder rejects it).  The blobs below are built from explicit
(code, z) lists, independent of any encoder, and decoded by `ref_decode`: zig-zag to int64 deltas, cumsum, low 16 bits.

Entries that pin the two prologue / tile fixes of the device decoders:
  * count_ffffffff_L4 (and the other count_fffffffX_* entries), count_exceeds_data: a count the blob cannot hold.  The key count
    used to be computed in 32 bits (0 for n >= 0xFFFFFFFD) and the count never checked against the data area, so these came back as
    status 6 ("signal slot too small", n_samples ~ 4.29 G) and the host retried with a slot of that size.  They must be 7.
  * overclaim_first_tile_*: the keys of the first tiles claim more data bytes than the blob has while the count still fits.  The
    staged tile copy (svb_decode_tile, svb_decode_tile_wave<true>) must load nothing once the data pointer is past the blob end;
    the status was 7 before and after, so that fix is checked by reading, with these entries driving it.
"""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import oracle_bind as ob
from deflate_craft import Bits
from signal_craft import WIDTH_END, WIDTH_LO, _interleave, svb_blob   # noqa: F401  (the builders: tests/signal_craft.py)
from signal_craft import svb_full_width as _full_width, svb_ref_decode as ref_decode

HDR_ARGS = (8192.0, 23.0, 1467.61, 4000.0)

def _small(rng, n, code3_at=()):
    """mostly one-byte deltas, a few two-byte ones; code-3 values at the given positions"""
    codes = np.where(rng.random(n) < 0.03, 1, 0).astype(np.uint8)
    for p in code3_at:
        codes[p] = 3
    return codes, _full_width(rng, codes)


SIZES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
CODE3_AT = (0, 15, 16, 1023, 1024, 4095, 4096)


def _corpus():
    """[(name, blob)]: valid small blobs, malformed blobs, then the long valid ones (so every malformed blob has long records
    behind it in a batch)"""
    rng = np.random.default_rng(0x5B2D)
    small, bad, big = [], [], []
    small.append(("zero_samples", svb_blob([], [])))
    codes = rng.integers(0, 4, 3000).astype(np.uint8)
    small.append(("random_codes_full_width", svb_blob(codes, _full_width(rng, codes))))
    codes = rng.integers(0, 4, 2000).astype(np.uint8)
    small.append(("non_minimal_widths", svb_blob(codes, rng.integers(0, 256, 2000).astype(np.uint64))))
    small.append(("z5_in_four_bytes", svb_blob([3, 3, 0, 3, 2], [5, 5, 5, 0, 1])))
    ext = np.array([0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE, 1, 0xFFFFFFFF, 0x80000000] * 40,
                   dtype=np.uint64)
    small.append(("extreme_z", svb_blob(np.full(len(ext), 3), ext)))
    # d = +2^31 - 1 again and again: the running sum wraps int32 (and int16) many times
    small.append(("sum_wraps_int32", svb_blob(np.full(700, 3), np.full(700, 0xFFFFFFFE, dtype=np.uint64))))
    small.append(("sum_wraps_int16", svb_blob(np.full(900, 1), np.full(900, 0xFFFE, dtype=np.uint64))))   # +32767 each step

    good = svb_blob(*_small(rng, 1500))
    bad += [("L0", b""), ("L1", good[:1]), ("L2", good[:2]), ("L3", good[:3])]
    bad.append(("one_trailing_byte", good + b"\x00"))
    bad.append(("one_data_byte_short", good[:-1]))
    bad.append(("key_area_longer_than_L", struct.pack("<I", 100) + bytes(10)))
    for n in (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF):
        for L in (4, 5, 8, 12, 16):
            bad.append(("count_%08x_L%d" % (n, L), struct.pack("<I", n) + bytes([0xFF]) * (L - 4)))
    bad.append(("count_2p30_L64", struct.pack("<I", 1 << 30) + bytes(60)))
    c, z = _small(rng, 1000)
    bad.append(("count_exceeds_data", svb_blob(c[:600], z[:600], count=1000)))   # keys for 1000 values fit, 600 data bytes do not
    # count, keys and n data bytes all fit, but the keys of the first tile(s) claim 4 bytes per value: the data runs out long before
    # the last tile (block tiles of 4096 values, wave tiles of 1024)
    for n, name in ((12288, "overclaim_first_tile_block"), (6144, "overclaim_first_tile_wave")):
        codes = np.zeros(n, dtype=np.uint8)
        codes[:4096 if n == 12288 else 1024] = 3
        bad.append((name, svb_blob(codes, _full_width(rng, codes))[:4 + n // 4 + n]))
    # data ends exactly at a tile boundary, values left behind it (random data bytes here and above: a zlib stream of runs would be
    # declined by the parallel inflate, and these blobs are meant for the staged wave tiles behind it too)
    codes = np.ones(4096 + 1000, dtype=np.uint8)
    codes[4096:] = 0
    blob = svb_blob(codes, _full_width(rng, codes))
    bad.append(("data_ends_at_block_tile", blob[:4 + len(codes) // 4 + 2 * 4096]))
    codes = np.zeros(1024 + 2000, dtype=np.uint8)
    codes[:1024] = 3
    blob = svb_blob(codes, _full_width(rng, codes))
    bad.append(("data_ends_at_wave_tile", blob[:4 + len(codes) // 4 + 4 * 1024]))

    for n in SIZES:
        codes = rng.integers(0, 4, n).astype(np.uint8)
        big.append(("n%d" % n, svb_blob(codes, _full_width(rng, codes))))
    for p in CODE3_AT:
        big.append(("code3_at_%d" % p, svb_blob(*_small(rng, 8200, code3_at=(p,)))))
    for n in (4096, 8192, 12289):   # 4 data bytes per value: a block tile fills its stage exactly
        codes = np.full(n, 3, dtype=np.uint8)
        big.append(("all_code3_n%d" % n, svb_blob(codes, _full_width(rng, codes))))
    return small + bad + big


CORPUS = _corpus()
REF = {name: ref_decode(blob) for name, blob in CORPUS}
MALFORMED = {name for name, _ in CORPUS if REF[name] is None}
# the entries that flip from 6 to 7 with the prologue fix when the signal slot is sized by the blob's bytes
BAD_COUNT = {name for name, _ in CORPUS if name.startswith("count_fffffff") or name == "count_exceeds_data"}


def _guards(k):
    """valid, short blobs that sit between the corpus entries of a batch"""
    rng = np.random.default_rng(0x6A5D + k)
    return [svb_blob(*_small(rng, int(rng.integers(200, 900)))) for _ in range(k)]


# ---------------------------------------------------------------- CPU: the reference against the oracle

def test_corpus_has_every_promised_shape():
    names = {n for n, _ in CORPUS}
    assert {"n%d" % n for n in SIZES} <= names and {"code3_at_%d" % p for p in CODE3_AT} <= names
    assert {"L0", "L1", "L2", "L3", "count_ffffffff_L4", "count_2p30_L64", "overclaim_first_tile_block", "overclaim_first_tile_wave",
            "data_ends_at_block_tile", "data_ends_at_wave_tile", "one_trailing_byte", "one_data_byte_short"} <= MALFORMED
    valid = [n for n, _ in CORPUS if n not in MALFORMED]
    assert len(valid) == len(CORPUS) - len(MALFORMED) and "zero_samples" in valid and "all_code3_n12289" in valid
    # the overclaiming blobs pass the count test and fail only on their data bytes
    for name in ("overclaim_first_tile_block", "overclaim_first_tile_wave", "data_ends_at_block_tile", "data_ends_at_wave_tile"):
        blob = dict(CORPUS)[name]
        n = struct.unpack_from("<I", blob)[0]
        assert 4 + (n + 3) // 4 + n <= len(blob), name


@pytest.mark.parametrize("name", [n for n, _ in CORPUS])
def test_reference_equals_the_oracle(name):
    blob = dict(CORPUS)[name]
    want = REF[name]
    try:
        got = ob.svbzd_decode(blob)
    except ValueError:
        got = None
    if want is None:
        assert got is None, name
    else:
        assert got is not None and np.array_equal(got, want), name
        # and the other way round: the oracle's encoding of those samples decodes to them
        enc = ob.svbzd_encode(want)
        assert np.array_equal(ref_decode(enc), want) and np.array_equal(ob.svbzd_decode(enc), want)


def test_builder_at_minimal_width_is_the_encoder():
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, 1000, 4097):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        d = np.diff(np.concatenate([[0], x.astype(np.int64)]))
        z = ((d << 1) ^ (d >> 63)).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        codes = (z > 0xFF).astype(np.uint8) + (z > 0xFFFF) + (z > 0xFFFFFF)
        assert svb_blob(codes, z) == ob.svbzd_encode(x)
        assert np.array_equal(ref_decode(svb_blob(codes, z)), x)


def test_reference_wraps_like_the_c_decoder():
    """a code-3 delta sum that leaves int32: the oracle accumulates modulo 2^32 and keeps the low 16 bits"""
    blob = svb_blob([3, 3, 3], [0xFFFFFFFE, 0xFFFFFFFE, 0x00000003])      # +2^31-1, +2^31-1, -2
    want = np.array([-1, -2, -4], dtype=np.int16)
    assert np.array_equal(ref_decode(blob), want) and np.array_equal(ob.svbzd_decode(blob), want)


# ---------------------------------------------------------------- GPU routes

def _payload(blob, i):
    from slow5tools_amd import press
    return press.pack_hdr(b"rd%d" % i, i, *HDR_ARGS) + struct.pack("<Q", len(blob)) + blob + _aux(i)


def _aux(i):
    return bytes([0xA0 + i % 16, i % 251, 0x5C])


def _check(name, status, n_samples, signal, aux=None, want_aux=None):
    want = REF.get(name) if isinstance(name, str) else name
    if want is None:
        assert status == 7, (name, status)
    else:
        assert status == 0, (name, status)
        assert n_samples == len(want) and np.array_equal(signal, want), name
        if want_aux is not None:
            assert aux == want_aux, name


def _batch():
    """(names, blobs): the corpus between guards; names of guards are their reference signals"""
    g = _guards(len(CORPUS) + 1)
    blobs = _interleave([b for _, b in CORPUS], g)
    names = _interleave([n for n, _ in CORPUS], [ref_decode(x) for x in g])
    return names, blobs


SENT = 0x5A5A


def _dev_decode(recs, form, sig_caps, rec_method=0, pay_caps=None, np_cap=None, n_slots=3, max_in_len=0, sig_method=1):
    """One device call on buffers laid out here.  form "blob": s5gpu_svbzd_decode_dev (recs are blobs); "full": s5gpu_decode_dev;
    "np": s5gpu_decode_dev with S5GPU_DEC_NO_PAYLOAD, n_slots scratch slots of np_cap, filled with 0xA5 beforehand.  Every signal slot
    is followed by at least 8 sentinel samples, which must survive.  Returns (fields, signals, payload or scratch buffer)."""
    import torch
    from slow5tools_amd import _lib
    L = _lib.lib()
    n = len(recs)
    lens = np.array([len(r) for r in recs], dtype=np.int64)
    in_off = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)]).astype(np.int64)
    blob = np.zeros(int(in_off[-1]) + 64, dtype=np.uint8)
    for r, o in zip(recs, in_off[:-1]):
        blob[o:o + len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
    caps = np.asarray(sig_caps, dtype=np.int64)
    sig_off = np.concatenate([[0], np.cumsum((caps + 15) // 8 * 8)]).astype(np.int64)
    d = np.zeros(n, dtype=_lib.REC_DESC)
    d["in_off"], d["in_len"], d["sig_off"], d["sig_cap"] = in_off[:-1], lens, sig_off[:-1], caps
    a = _lib.DecodeArgs()
    a.n_recs, a.rec_method, a.sig_method = n, rec_method, sig_method
    dev = torch.device("cuda:0")
    if form == "full":
        pc = np.asarray(pay_caps, dtype=np.int64)
        pay_off = np.concatenate([[0], np.cumsum((pc + 31) // 16 * 16)]).astype(np.int64)
        d["pay_off"], d["pay_cap"] = pay_off[:-1], pc
        pay = torch.zeros(int(pay_off[-1]) + 64, dtype=torch.uint8, device=dev)
        a.max_pay_cap = int(pc.max())
    elif form == "np":
        slot = (np_cap + 16 + 15) & ~15
        pay = torch.full((64 + n_slots * slot,), 0xA5, dtype=torch.uint8, device=dev)
        a.flags, a.max_pay_cap, a.payload_bytes, a.max_in_len = _lib.DEC_NO_PAYLOAD, np_cap, 64 + n_slots * slot, max_in_len
    else:
        pay = None
    t_in = torch.from_numpy(blob).to(dev)
    t_desc = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
    t_sig = torch.full((int(sig_off[-1]) + 64,), SENT, dtype=torch.int16, device=dev)
    t_fields = torch.zeros(max(n, 1) * _lib.REC_FIELDS.itemsize, dtype=torch.uint8, device=dev)
    a.desc, a.in_, a.sig_out, a.fields = t_desc.data_ptr(), t_in.data_ptr(), t_sig.data_ptr(), t_fields.data_ptr()
    if pay is not None:
        a.payload = pay.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if form == "blob":
        _lib.check(L.s5gpu_svbzd_decode_dev(C.byref(a), st), "s5gpu_svbzd_decode_dev")
    else:
        _lib.check(L.s5gpu_decode_dev(C.byref(a), st), "s5gpu_decode_dev")
    torch.cuda.synchronize(dev)
    f = t_fields.cpu().numpy().view(_lib.REC_FIELDS)[:n].copy()
    sig = t_sig.cpu().numpy()
    for i in range(n):   # nothing written behind a signal slot
        assert (sig[sig_off[i] + caps[i]:sig_off[i + 1]] == SENT).all(), i
    out = [sig[sig_off[i]:sig_off[i] + int(f["n_samples"][i])].copy() if f["status"][i] == 0 else None for i in range(n)]
    return f, out, (pay.cpu().numpy() if pay is not None else None)


def _sig_caps(names, blobs):
    """valid: exactly the samples; malformed: the blob's byte count (what a caller sizing by the blob would give: a count the blob
    cannot hold does not fit it)"""
    return [len(REF[nm] if isinstance(nm, str) else nm) if (not isinstance(nm, str) or REF[nm] is not None) else len(b)
            for nm, b in zip(names, blobs)]


@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


def _opt(key, value):
    from slow5tools_amd import _lib
    _lib.check(_lib.lib().s5gpu_set_option(key, value), "s5gpu_set_option")


@pytest.mark.gpu
def test_blob_kernel_direct_call(press):
    """k_svbzd_decode: s5gpu_svbzd_decode_dev launches it and nothing else"""
    names, blobs = _batch()
    f, sig, _ = _dev_decode(blobs, "blob", _sig_caps(names, blobs))
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
        if f["status"][i] == 0:
            assert f["payload_len"][i] == len(blobs[i])
    assert {nm for i, nm in enumerate(names) if isinstance(nm, str) and f["status"][i] == 7} == MALFORMED


@pytest.mark.gpu
def test_solo_depress_batch_and_single_calls(press):
    """slow5_ptr_depress_solo(SVB_ZD) and its batch form (s5gpu_solo_batch stage 3: the host sizes each slot from the blob's count,
    retries a status 6 with the count reported, and decodes with k_svbzd_decode)"""
    from slow5tools_amd import _lib
    L = _lib.lib()
    names, blobs = _batch()
    n = len(blobs)
    bufs = [C.create_string_buffer(b, max(len(b), 1)) for b in blobs]
    inp = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    out, olen, st = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int32 * n)()
    rc = L.s5gpu_solo_batch(3, n, inp, lens, out, olen, st)
    assert rc == -5    # S5GPU_ERR_DATA: some inputs are corrupt
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for i, nm in enumerate(names):
        s = np.frombuffer(C.string_at(out[i], olen[i]), dtype=np.int16) if out[i] else None
        _check(nm, st[i], olen[i] // 2, s)
        if out[i]:
            libc.free(out[i])
    L.slow5_ptr_depress_solo.restype = C.c_void_p
    L.slow5_ptr_depress_solo.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    SVB = 2
    for name, blob in CORPUS:
        cnt = C.c_size_t(12345)
        p = L.slow5_ptr_depress_solo(SVB, blob, len(blob), C.byref(cnt))
        if REF[name] is None:
            assert not p, name
        else:
            assert p and cnt.value == 2 * len(REF[name]), name
            assert np.array_equal(np.frombuffer(C.string_at(p, cnt.value), dtype=np.int16), REF[name]), name
            libc.free(p)


def _records(names, blobs):
    return [_payload(b, i) for i, b in enumerate(blobs)]


def _check_host(names, recs_out, pays=None):
    for i, (nm, g) in enumerate(zip(names, recs_out)):
        _check(nm, g["status"], len(g.get("signal", ())), g.get("signal"), g.get("aux"), _aux(i))
        if g["status"] == 0:
            assert g["read_group"] == i and g["read_id"] == b"rd%d" % i
            if pays is not None:
                assert g["payload"] == pays[i]


@pytest.mark.gpu
def test_workgroup_unpack_kernel(press):
    """k_unpack: records without a record press (k_inflate only copies them; nothing but k_unpack unpacks REC_NONE), and zlib
    records with unpack_fused = 0 (k_inflate_par<0> / fallback, then k_unpack)"""
    names, blobs = _batch()
    pays = _records(names, blobs)
    _check_host(names, press.decode_records(pays, press.REC_NONE, press.SIG_SVB_ZD, raise_on_error=False), pays)
    streams = [zlib.compress(p, 6) for p in pays]
    _opt(b"unpack_fused", 0)
    try:
        _check_host(names, press.decode_records(streams, raise_on_error=False), pays)
    finally:
        _opt(b"unpack_fused", 1)


@pytest.mark.gpu
def test_fused_wave_unpack_behind_the_parallel_inflate(press):
    """k_inflate_par<1>: zlib records, default options — the wave that inflates a record unpacks it (svb_decode_tile_wave<true>,
    staged).  That the parallel decoder takes every one of these records: with inflate_par = 2 (no fallback pass) none reports 8."""
    names, blobs = _batch()
    pays = _records(names, blobs)
    streams = [zlib.compress(p, 6) for p in pays]
    _check_host(names, press.decode_records(streams, raise_on_error=False), pays)
    _opt(b"inflate_par", 2)
    try:
        alone = press.decode_records(streams, raise_on_error=False)
    finally:
        _opt(b"inflate_par", 1)
    assert not [i for i, g in enumerate(alone) if g["status"] == 8]
    _check_host(names, alone, pays)


# 8 MiB of zeros: stock zlib codes the run as length-258, distance-1 matches of 2 bits each, several windows of them, so a round of
# the parallel decoder comes to start a full-window segment (511 bits: 256 matches, 66 048 bytes) inside the run — more than the
# 64 KiB one segment may expand to, and the record is declined (INF_NEED_FALLBACK) to the wave decoder
RUN_AUX = bytes(8 << 20)


@pytest.mark.gpu
def test_fallback_inflate_then_unpack_rest(press):
    """k_inflate_fallback + k_unpack_rest: the malformed entries and a set of valid ones, each record with a long run of zeros in its
    aux field (declined by the parallel decoder: inflate_par = 2 leaves status 8 on each), between short guards that the parallel
    decoder takes and unpacks itself — k_unpack_rest must pick exactly the others"""
    keep = [(n, b) for n, b in CORPUS if n in MALFORMED or n in ("zero_samples", "n17", "n4097", "code3_at_4096", "all_code3_n4096",
                                                                   "extreme_z")]
    g = _guards(len(keep) + 1)
    names = _interleave([n for n, _ in keep], [ref_decode(x) for x in g])
    blobs = _interleave([b for _, b in keep], g)
    pays = []
    for i, (nm, b) in enumerate(zip(names, blobs)):
        p = _payload(b, i)
        pays.append(p + RUN_AUX if isinstance(nm, str) else p)
    streams = [zlib.compress(p, 6) for p in pays]
    got = press.decode_records(streams, raise_on_error=False)
    for i, (nm, r) in enumerate(zip(names, got)):
        _check(nm, r["status"], len(r.get("signal", ())), r.get("signal"), r.get("aux"), (_aux(i) + RUN_AUX) if isinstance(nm, str) else _aux(i))
    del got
    _opt(b"inflate_par", 2)
    try:
        alone = press.decode_records(streams, raise_on_error=False)
    finally:
        _opt(b"inflate_par", 1)
    routed = [isinstance(nm, str) for nm in names]
    assert [g_["status"] == 8 for g_ in alone] == routed


def _np_cap(pays):
    return max(len(p) for p in pays) + 64


@pytest.mark.gpu
def test_no_payload_slot_form(press):
    """k_inflate_par_np (np_lds_payload = 0): each record is inflated into its workgroup's scratch slot and unpacked from there.
    Three slots of scratch: two for the main kernel, one for k_inflate_fallback_np — that one stays untouched (no record declined),
    the two main ones hold payload bytes"""
    names, blobs = _batch()
    pays = _records(names, blobs)
    streams = [zlib.compress(p, 6) for p in pays]
    cap = _np_cap(pays)
    _opt(b"np_lds_payload", 0)
    try:
        f, sig, scr = _dev_decode(streams, "np", _sig_caps(names, blobs), rec_method=1, np_cap=cap, max_in_len=max(map(len, streams)))
    finally:
        _opt(b"np_lds_payload", 1)
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
        if f["status"][i] == 0:
            assert f["aux_len"][i] == 3 and f["read_group"][i] == i
    slot = (cap + 31) & ~15
    assert (scr[64 + 2 * slot:64 + 3 * slot] == 0xA5).all()
    assert (scr[64:64 + slot] != 0xA5).any() and (scr[64 + slot:64 + 2 * slot] != 0xA5).any()


def _fixed_literals(p):
    """a zlib stream of one final fixed-code block of literals only (RFC 1951 3.2.6).  zlib itself turns a near-random payload into
    a stored block even with Z_FIXED, and the LDS kernel declines stored blocks"""
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    for c in p:
        if c < 144:
            b.put_code(0x30 + c, 8)
        else:
            b.put_code(0x190 + c - 144, 9)
    b.put_code(0, 7)
    s = b"\x78\x01" + b.done() + struct.pack(">I", zlib.adler32(p))
    assert zlib.decompress(s) == p
    return s


def _fits_one_window(p):
    """the stream of a payload for k_inflate_par_np_lp (a record of one inflate window, max_in_len <= IP_SPAN - 96), or None"""
    if len(p) > 3600:
        return None
    s = _fixed_literals(p)
    return s if len(s) <= 3900 else None


@pytest.mark.gpu
def test_no_payload_lds_form_and_its_fallback(press):
    """k_inflate_par_np_lp: the records of one inflate window (max_in_len <= IP_SPAN - 96; fixed-code literal streams of short payloads) are
    inflated into LDS and unpacked there (svb_decode_tile_wave<false>): no byte of scratch is written.  The same payloads as stored
    blocks, which that kernel declines before writing anything: k_inflate_fallback_np inflates them into its slot (the third of
    three) and unpacks them there — the slot then holds the last of them."""
    names, blobs = _batch()
    pays = _records(names, blobs)
    sel = [i for i, p in enumerate(pays) if _fits_one_window(p) is not None]
    assert len(sel) > 60 and {n for i, n in enumerate(names) if i in sel and isinstance(n, str)} >= {
        "zero_samples", "L0", "count_ffffffff_L4", "count_2p30_L64", "n1023", "n1025", "z5_in_four_bytes", "extreme_z"}
    names = [names[i] for i in sel]
    blobs = [blobs[i] for i in sel]
    pays = [pays[i] for i in sel]
    cap = 5344
    slot = (cap + 31) & ~15
    fixed = [_fits_one_window(p) for p in pays]
    f, sig, scr = _dev_decode(fixed, "np", _sig_caps(names, blobs), rec_method=1, np_cap=cap, max_in_len=4000)
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
    assert (scr[64:64 + 3 * slot] == 0xA5).all()
    stored = [zlib.compress(p, 0) for p in pays]
    f, sig, scr = _dev_decode(stored, "np", _sig_caps(names, blobs), rec_method=1, np_cap=cap, max_in_len=4000)
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
    assert (scr[64:64 + 2 * slot] == 0xA5).all()
    last = pays[-1]
    assert bytes(scr[64 + 2 * slot:64 + 2 * slot + len(last)]) == last


@pytest.mark.gpu
def test_zstd_full_and_no_payload_forms(press):
    """k_zstd_inflate<1> (decode_records on zstd frames: the decoding wave unpacks; and unpack_fused = 0, k_unpack behind
    k_zstd_inflate<0>) and k_zstd_inflate_np (no-payload form: its scratch slots hold payload bytes afterwards)"""
    assert ob.zstd_ref() is not None
    names, blobs = _batch()
    pays = _records(names, blobs)
    frames = [ob.zstd_compress(p) for p in pays]
    _check_host(names, press.decode_records(frames, press.REC_ZSTD, raise_on_error=False), pays)
    _opt(b"unpack_fused", 0)
    try:
        _check_host(names, press.decode_records(frames, press.REC_ZSTD, raise_on_error=False), pays)
    finally:
        _opt(b"unpack_fused", 1)
    cap = _np_cap(pays)
    f, sig, scr = _dev_decode(frames, "np", _sig_caps(names, blobs), rec_method=2, np_cap=cap)
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
    assert (scr[64:64 + ((cap + 31) & ~15)] != 0xA5).any()


@pytest.mark.gpu
def test_zero_sample_read_on_every_route(press):
    """an empty signal from our own encoder and the hand-made n = 0, L = 4 blob: an empty signal everywhere, fields as the CPU parser
    has them (a blob of fewer than 4 bytes is malformed everywhere: the corpus entries L0..L3)"""
    hdr = press.pack_hdr(b"empty", 7, *HDR_ARGS)
    own = press.encode_records([np.zeros(0, np.int16)], [hdr], [b"xy"])[0][8:]
    want = ob.rec_parse(zlib.decompress(own), ob.SIG_SVB_ZD)
    assert len(want["signal"]) == 0
    hand = zlib.compress(hdr + struct.pack("<Q", 4) + b"\x00\x00\x00\x00" + b"xy")
    assert zlib.decompress(hand) == zlib.decompress(own)
    guard = zlib.compress(_payload(_guards(1)[0], 0))
    recs = [guard, own, hand, guard]
    for fused in (1, 0):
        _opt(b"unpack_fused", fused)
        try:
            got = press.decode_records(recs)
        finally:
            _opt(b"unpack_fused", 1)
        for g in got[1:3]:
            assert g["status"] == 0 and len(g["signal"]) == 0 and g["aux"] == want["aux"] and g["read_id"] == want["read_id"]
            assert g["read_group"] == want["read_group"] and g["range"] == want["range"]
    for lds in (1, 0):
        _opt(b"np_lds_payload", lds)
        try:
            f, s = press.decode_signals_dev(recs, max_pay_cap=4096, sig_caps=[2000, 0, 0, 2000], max_in_len=4000)
        finally:
            _opt(b"np_lds_payload", 1)
        assert list(f["status"]) == [0, 0, 0, 0] and list(f["n_samples"][1:3]) == [0, 0] and list(f["aux_len"][1:3]) == [2, 2]
    zs = [ob.zstd_compress(zlib.decompress(r)) for r in recs]
    got = press.decode_records(zs, press.REC_ZSTD)
    assert all(g["status"] == 0 for g in got) and len(got[1]["signal"]) == len(got[2]["signal"]) == 0


@pytest.mark.gpu
def test_valid_blob_in_too_small_a_signal_slot(press):
    """a signal slot one sample short: the device calls report 6 with the blob's count (k_svbzd_decode, k_unpack, k_inflate_par<1>,
    k_inflate_par_np, k_inflate_par_np_lp); the host batches size their slots from the payload and decode the same blobs"""
    pick = ["n1", "n17", "n1025", "n4097", "code3_at_4096", "all_code3_n4096", "extreme_z"]
    blobs = [dict(CORPUS)[n] for n in pick]
    g = _guards(len(pick) + 1)
    all_blobs = _interleave(blobs, g)
    wants = _interleave([REF[n] for n in pick], [ref_decode(x) for x in g])
    short = [len(w) - 1 if k % 2 else len(w) for k, w in enumerate(wants)]

    def check6(f, sig):
        for k, w in enumerate(wants):
            if k % 2:
                assert f["status"][k] == 6 and f["n_samples"][k] == len(w), (k, int(f["status"][k]))
            else:
                assert f["status"][k] == 0 and np.array_equal(sig[k], w), k

    check6(*_dev_decode(all_blobs, "blob", short)[:2])
    pays = [_payload(b, i) for i, b in enumerate(all_blobs)]
    check6(*_dev_decode(pays, "full", short, rec_method=0, pay_caps=[len(p) + 64 for p in pays])[:2])
    streams = [zlib.compress(p, 6) for p in pays]
    check6(*_dev_decode(streams, "full", short, rec_method=1, pay_caps=[len(p) + 64 for p in pays])[:2])
    cap = _np_cap(pays)
    _opt(b"np_lds_payload", 0)
    try:
        check6(*_dev_decode(streams, "np", short, rec_method=1, np_cap=cap, max_in_len=max(map(len, streams)))[:2])
    finally:
        _opt(b"np_lds_payload", 1)
    small = [k for k, p in enumerate(pays) if _fits_one_window(p) is not None]
    assert len(small) >= 5
    f, s, scr = _dev_decode([_fits_one_window(pays[k]) for k in small], "np", [short[k] for k in small], rec_method=1, np_cap=5344,
                            max_in_len=4000)
    for j, k in enumerate(small):
        if k % 2:
            assert f["status"][j] == 6 and f["n_samples"][j] == len(wants[k]), k
        else:
            assert f["status"][j] == 0 and np.array_equal(s[j], wants[k]), k
    assert (scr[64:] == 0xA5).all()                            # (the LDS kernel took them all)
    # host batches: the same blobs come back whole
    from slow5tools_amd import _lib
    L = _lib.lib()
    L.slow5_ptr_depress_solo.restype = C.c_void_p
    L.slow5_ptr_depress_solo.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for b, w in zip(all_blobs, wants):
        cnt = C.c_size_t()
        p = L.slow5_ptr_depress_solo(2, b, len(b), C.byref(cnt))
        assert p and np.array_equal(np.frombuffer(C.string_at(p, cnt.value), dtype=np.int16), w)
        libc.free(p)
    for got in (press.decode_records(pays, press.REC_NONE, press.SIG_SVB_ZD), press.decode_records(streams)):
        assert all(gg["status"] == 0 and np.array_equal(gg["signal"], w) for gg, w in zip(got, wants))
    f, s = press.decode_signals_dev(streams, max_pay_cap=cap, sig_caps=[len(w) for w in wants])
    assert all(f["status"] == 0) and all(np.array_equal(x, w) for x, w in zip(s, wants))
