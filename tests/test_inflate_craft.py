"""Every route of the zlib record decoders on hand-made DEFLATE streams (tests/deflate_craft.py).  Valid streams carry the bytes the
builder got by executing its own tokens; stock zlib (`zlib.decompressobj(15)`: decompresses, eof, nothing left over) is the referee of
what is a stream at all, and a plain-Python inflate written from the RFCs stands beside it.  The CPU tests pin the catalogue, the Python
inflate and the mutant set on stock zlib; the GPU tests put the same streams through

  route         options                                            kernels
  wave          inflate_par 0, inflate_simt_min huge               k_inflate (zlib_inflate_wave, csrc/inflate_dev.h)
  lane          inflate_par 0, inflate_simt_min 1, inflate_route 0 k_inflate_simt<false> (zlib_inflate_lane, csrc/inflate_simt_dev.h)
  lane_routed   ... inflate_route 1, >= 1024 records               k_inflate_simt<true>, and k_inflate_long for records of >= 32 KiB
  par           inflate_par 1 (the default)                        k_inflate_par<0> (zlib_inflate_par, csrc/inflate_par_dev.h) + k_inflate_fallback
  par_alone     inflate_par 2                                      k_inflate_par<0> without the fallback: 8 = declined
  head          s5gpu_inflate_head_dev                             k_inflate_head (zlib_inflate_wave<HEAD>)
  host          decode_records, s5gpu_solo_batch(1), slow5_ptr_depress_solo(ZLIB)     the default kernels behind the host's slot sizing and retries
  records       s5gpu_decode_dev: full form, both list shapes      k_inflate_par<1 | 2, SHORT> / <.., false>, k_unpack, k_unpack_rest
                S5GPU_DEC_NO_PAYLOAD, max_in_len <= 4000           k_inflate_par_np_lp + k_inflate_fallback_np
                S5GPU_DEC_NO_PAYLOAD, max_in_len unknown           k_inflate_par_np + k_inflate_fallback_np
"""
import contextlib
import ctypes as C
import functools
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as dc

ZV = "zlib " + zlib.ZLIB_RUNTIME_VERSION          # in every failure message: the referee is whatever zlib this Python runs on
REJECT_ROOM = 1024                                # payload slot of a malformed stream: what it produced before its fault + this

# ---------------------------------------------------------------- the names the catalogue promises (written out, not generated from it)
PROMISED_VALID = (
    ["len_sym_%d" % s for s in range(257, 286)] + ["len_258_as_284_plus_31", "len_258_as_285"] + ["dist_sym_%d" % s for s in range(30)]
    + ["far_d%d_l%d" % (d, l) for d in (32506, 32507, 32767, 32768) for l in (3, 258)]
    + ["dist_eq_out_%d" % k for k in (1, 2, 3, 4, 5, 64, 258, 259, 2047, 2048, 2049, 4095, 4096, 4097)]
    + ["overlap_d%d_o%d" % (d, o) for d in (1, 2, 3, 4) for o in range(4)] + ["dist_4095", "dist_4096", "dist_4097"]
    + ["match_source_spans_block_boundary", "match_source_spans_stored_block", "match_destination_spans_flush", "match_behind_stored_copies_it"]
    + ["empty_fixed_block", "empty_dynamic_block_eob_only", "empty_blocks_1_then_data", "empty_blocks_2_then_data", "empty_blocks_40_then_data"]
    + ["stored_len%d_bit%d" % (n, k) for n in (0, 1, 65535) for k in range(8)] + ["stored_between_huffman_blocks"]
    + ["final_stored_block_bit0", "final_stored_block_bit5", "final_stored_block_empty"]
    + ["final_block_ends_on_a_byte", "final_block_ends_on_the_2048_window", "final_block_ends_on_the_4096_window"]
    + ["token48_across_the_2048_window", "token48_across_the_4096_window"]
    + ["hdist1_length0_literals_only", "single_distance_code_of_1_bit", "distance_codes_30_complete", "distance_codes_of_15_bits"]
    + ["litlen_codes_up_to_9_bits", "litlen_long_codes_under_one_prefix", "litlen_long_codes_under_many_prefixes", "longest_code_first_in_a_segment"]
    + ["all_286_litlen_symbols_in_use", "fixed_code_range_edges"]
    + ["segments_span_%d" % (384 * k + d) for k in (1, 2, 63, 64) for d in (-1, 0, 1)]
    + ["end_of_block_first_in_a_segment", "dynamic_header_longer_than_a_segment", "more_waiting_matches_than_the_list_holds"]
    + ["cinfo0_far_distances", "cinfo7_far_distances"] + ["flevel%d_far_distances" % k for k in range(4)])
PROMISED_MALFORMED = {
    "header_cm_7": 1, "header_cinfo_8": 1, "header_bad_fcheck": 1, "header_fdict": 1,
    "block_type_3": 2, "stored_nlen_mismatch": 2, "stored_len_past_the_end": 3,
    "fixed_litlen_symbol_286": 2, "fixed_litlen_symbol_287": 2, "fixed_distance_symbol_30": 2, "fixed_distance_symbol_31": 2,
    "hlit_287": 2, "hlit_288": 2, "hdist_31": 2, "hdist_32": 2,
    "code_length_code_oversubscribed": 2, "code_length_code_incomplete": 2, "litlen_code_oversubscribed": 2, "litlen_code_incomplete": 2,
    "litlen_single_code_of_2_bits": 2, "distance_code_oversubscribed": 2, "distance_code_incomplete": 2, "distance_single_code_of_2_bits": 2,
    "distance_codes_30_of_5_bits": 2, "no_end_of_block_code": 2, "length_symbol_without_distance_code": 2,
    "too_far_first_token": 2, "too_far_after_1_literals": 2, "too_far_after_5_literals": 2, "too_far_after_258_literals": 2,
    "too_far_after_4097_literals": 2, "too_far_behind_stored_block": 2, "too_far_32768_with_32767_out": 2, "too_far_in_a_later_window": 2,
    "bad_adler": 4, "byte_between_last_block_and_adler": 4, "bytes_behind_the_adler": None, "no_final_block": 3,
    "cut_to_1_bytes": 3, "cut_to_2_bytes": 3, "cut_to_5_bytes": 3,
    # a cut reports 3 at every structural place: what the bits behind the end would have said (LEN = NLEN = 0, an empty code-length code)
    # is not looked at
    "cut_in_block_header": 3, "cut_in_hlit_hdist_hclen": 3, "cut_in_code_length_code_lengths": 3, "cut_in_code_length_sequence": 3,
    "cut_in_literal": 3, "cut_in_length_code": 3, "cut_in_length_extra": 3, "cut_in_distance_code": 3, "cut_in_distance_extra": 3,
    "cut_in_end_of_block": 3, "cut_in_stored_len": 3, "cut_in_stored_nlen": 3, "cut_in_stored_bytes": 3, "cut_in_fixed_block_token": 3,
    "cut_in_last_end_of_block": 3, "cut_1_bytes_off_the_adler": 3, "cut_2_bytes_off_the_adler": 3, "cut_3_bytes_off_the_adler": 3,
    "cut_4_bytes_off_the_adler": 3}


# ---------------------------------------------------------------- CPU: catalogue, Python inflate, stock zlib
def test_catalogue_has_every_promised_name():
    cat = dc.by_name()
    assert len(cat) == len(dc.catalogue())
    missing = [n for n in PROMISED_VALID if n not in cat or cat[n].expected is None]
    assert not missing, missing
    wrong = [n for n, s in PROMISED_MALFORMED.items() if n not in cat or cat[n].expected is not None or cat[n].status != s]
    assert not wrong, wrong
    assert set(cat) == set(PROMISED_VALID) | set(PROMISED_MALFORMED)          # and nothing that no list names
    assert max(len(e.expected) for e in cat.values() if e.expected is not None) <= 70000
    assert all(e.why for e in cat.values())


def test_builder_python_inflate_and_stock_zlib_agree_on_the_catalogue():
    """valid: the bytes the builder executed = the Python inflate's (under zlib's framing and under the device's) = stock zlib's;
    malformed: both refuse, and the status the table names is the one the Python inflate derives under the device's framing"""
    for e in dc.catalogue():
        ref, mine, dev = dc.referee(e.stream), dc.py_inflate(e.stream), dc.py_inflate(e.stream, "device")
        if e.expected is not None:
            assert ref == e.expected, (e.name, ZV)
            assert mine.data == e.expected and dev.data == e.expected, (e.name, mine.reason, dev.reason)
        else:
            assert ref is None, (e.name, ZV)
            assert mine.data is None and mine.status != 0, e.name
            if e.status is not None:
                assert dev.data is None and dev.status == e.status, (e.name, dev.status, dev.reason)
    trailing = dc.by_name()["bytes_behind_the_adler"]
    assert dc.referee(trailing.stream[:-3]) is not None and dc.py_inflate(trailing.stream).gap == 3      # the stream in front of them is whole


def test_docs_list_every_entry_with_its_reason_and_status():
    """docs/codecs.md 4.7 has one table row per catalogue entry: | `name` | what it is for | status |"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "docs", "codecs.md"), encoding="utf-8").read()
    rows = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"^\| `(\w+)` \| (.*) \| (\d|—) \|$", text, re.M)}
    for e in dc.catalogue():
        assert rows.get(e.name) == (e.why, "—" if e.status is None else str(e.status)), e.name
    assert len(rows) == len(dc.catalogue())


def test_shapes_are_the_ones_the_names_promise():
    """the bit arithmetic behind a few names, checked on the Python inflate's marks"""
    cat = dc.by_name()
    for nbytes, name in ((18, "final_block_ends_on_a_byte"), (2048, "final_block_ends_on_the_2048_window"), (4096, "final_block_ends_on_the_4096_window")):
        assert dc.py_inflate(cat[name].stream).end_bit == 8 * nbytes == 8 * (len(cat[name].stream) - 6)
    for k in range(8):
        r = dc.py_inflate(cat["stored_len1_bit%d" % k].stream)
        stored = [i for i, (bit, n) in enumerate(r.marks) if i and bit - r.marks[i - 1][0] > 32 and n - r.marks[i - 1][1] == 1]
        assert len(stored) == 1 and (r.marks[stored[0] - 1][0] + 7) % 8 == k          # (+ 7: the end-of-block code of the fixed block in front)
    r = dc.py_inflate(cat["more_waiting_matches_than_the_list_holds"].stream)
    assert len(r.marks) == 4900 and r.marks[-1][0] - r.marks[3999][0] < 8 * 4096 - 64   # the 900 matches fit one round's window
    assert dc.py_inflate(cat["token48_across_the_2048_window"].stream).marks[-7][0] - dc.py_inflate(cat["token48_across_the_2048_window"].stream).marks[-8][0] == 48


# ---------------------------------------------------------------- mutants
N_MUTANTS = 600
MUTANT_SEED = 20
MUTANT_SHORT_SOURCE = 4200            # bytes of the longest stream in the pool of stored / fixed-only sources


def _with_adler_of_what_it_holds(g):
    """if the deflate data of g inflates on its own (raw, wbits -15), g cut behind its last block and given the Adler-32 of those bytes"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(bytes(g[2:]))
    except zlib.error:
        return g
    if not d.eof:
        return g
    used = len(g) - 2 - len(d.unused_data)
    return bytes(g[:2 + used]) + struct.pack(">I", zlib.adler32(out) & 0xFFFFFFFF)


def excluded(stream):
    """a deliberate difference from stock zlib, by a property the Python inflate computes from the stream: none today"""
    return False


@functools.lru_cache(maxsize=None)
def mutants():
    """[(source name, stream)]: valid catalogue streams with 1, 2 or 3 bytes changed, or cut short; every other one gets the Adler-32
    of what it now holds if its deflate data still inflates, so that accepting it means decoding OTHER bytes than the source's.  One in
    four comes from ANY valid stream of the catalogue, two from the streams of up to MUTANT_SHORT_SOURCE bytes that hold stored and fixed
    blocks only, one from the streams with a stored block of 65 535 bytes (a changed byte in a dynamic header or in Huffman data is
    refused nearly always: with an even draw over the short streams stock zlib accepted 88 of the 600, without the long stored blocks 98)"""
    rng = np.random.default_rng(MUTANT_SEED)
    src = [e for e in dc.catalogue() if e.expected is not None]
    plain = [e for e in src if len(e.stream) <= MUTANT_SHORT_SOURCE and 2 not in dc.py_inflate(e.stream).blocks]
    long_stored = [e for e in dc.catalogue() if e.name.startswith("stored_len65535")]
    assert len(plain) >= 50 and len(src) - len(plain) >= 10 and len(long_stored) == 8
    out = []
    while len(out) < N_MUTANTS:
        k = len(out)
        pool = src if k % 8 < 2 else long_stored if k % 8 < 4 else plain
        e = pool[int(rng.integers(0, len(pool)))]
        g = bytearray(e.stream)
        if k % 4 == 3:
            g = g[:int(rng.integers(1, len(g)))]
        else:
            for pos in rng.integers(0, len(g), 1 + k % 3):
                g[pos] = int(rng.integers(0, 256))
        g = bytes(g)
        if k % 2 == 0:
            g = _with_adler_of_what_it_holds(g)
        if g != e.stream:
            out.append((e.name, g))
    return out


@functools.lru_cache(maxsize=None)
def mutant_answers():
    return [dc.referee(g) for _, g in mutants()]


def test_mutants_are_classified_by_the_referee():
    M, ref = mutants(), mutant_answers()
    assert len(M) == N_MUTANTS
    n_ok = sum(r is not None for r in ref)
    assert n_ok >= 100 and N_MUTANTS - n_ok >= 100, (n_ok, ZV)
    assert sum(r is not None and r != dc.by_name()[name].expected for (name, _), r in zip(M, ref)) >= 50, ZV      # accepted with other bytes
    assert sum(excluded(g) for _, g in M) <= N_MUTANTS // 20
    for (name, g), r in zip(M, ref):                                                   # the Python inflate agrees with the referee on all of them
        mine = dc.py_inflate(g)
        assert mine.data == r, (name, mine.reason, ZV)


# ---------------------------------------------------------------- the device
SENT = 0xA5
DEFAULTS = {b"inflate_par": 1, b"inflate_simt_min": 24576, b"inflate_route": 1, b"unpack_fused": 1}
ROUTES = {"wave": {b"inflate_par": 0, b"inflate_simt_min": 1 << 30},
          "lane": {b"inflate_par": 0, b"inflate_simt_min": 1, b"inflate_route": 0},
          "lane_routed": {b"inflate_par": 0, b"inflate_simt_min": 1, b"inflate_route": 1},
          "par": {b"inflate_par": 1},
          "par_alone": {b"inflate_par": 2}}
FULL_ROUTES = ("wave", "lane", "lane_routed", "par")
# what the parallel decoder declines today (status 8 with inflate_par = 2: the wave decoder redoes these): a later change that declines more
# shows up here
DECLINED_TODAY = set()


@contextlib.contextmanager
def options(opts):
    from slow5tools_amd import _lib
    L = _lib.lib()
    try:
        for k, v in opts.items():
            _lib.check(L.s5gpu_set_option(k, v), "s5gpu_set_option")
        yield
    finally:
        for k, v in DEFAULTS.items():
            _lib.check(L.s5gpu_set_option(k, v), "s5gpu_set_option")


@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


def inflate_dev(streams, caps, head=False, in_lens=None):
    """One s5gpu_inflate_dev (head: s5gpu_inflate_head_dev) call on buffers laid out here, as test_svbzd_decode._dev_decode lays them out:
    the streams at 16-byte offsets (a stream cut at a multiple of 16 has the next one exactly where it would have continued), in_len as given
    (default: the whole stream); every payload slot of caps[i] bytes followed by at least 48 sentinel bytes, slots
    and sentinels filled with 0xA5 beforehand — the byte a read in front of a slot (the slot before it, or its sentinels) would show, and
    what must still stand at and beyond caps[i] afterwards.  Returns (status, payload_len, [bytes of each slot up to min(payload_len, cap)])."""
    import torch
    from slow5tools_amd import _lib
    L = _lib.lib()
    n = len(streams)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    in_off = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)]).astype(np.int64)
    blob = np.zeros(int(in_off[-1]) + 64, dtype=np.uint8)
    for s, o in zip(streams, in_off[:-1]):
        blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
    caps = np.asarray(caps, dtype=np.int64)
    pay_off = np.concatenate([[0], np.cumsum((caps + 15) // 16 * 16 + 48)]).astype(np.int64)
    d = np.zeros(n, dtype=_lib.REC_DESC)
    d["in_off"], d["in_len"], d["pay_off"], d["pay_cap"] = in_off[:-1], lens if in_lens is None else np.asarray(in_lens, dtype=np.int64), pay_off[:-1], caps
    dev = torch.device("cuda:0")
    t_in = torch.from_numpy(blob).to(dev)
    t_desc = torch.from_numpy(d.view(np.uint8).copy()).to(dev)
    t_pay = torch.full((int(pay_off[-1]) + 64,), SENT, dtype=torch.uint8, device=dev)
    t_fields = torch.full((n * _lib.REC_FIELDS.itemsize,), 0xEE, dtype=torch.uint8, device=dev)
    a = _lib.DecodeArgs()
    a.n_recs, a.rec_method, a.sig_method = n, 1, 1
    a.desc, a.in_, a.payload, a.fields = t_desc.data_ptr(), t_in.data_ptr(), t_pay.data_ptr(), t_fields.data_ptr()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if head:
        _lib.check(L.s5gpu_inflate_head_dev(C.byref(a), st), "s5gpu_inflate_head_dev")
    else:
        _lib.check(L.s5gpu_inflate_dev(C.byref(a), st), "s5gpu_inflate_dev")
    torch.cuda.synchronize(dev)
    f = t_fields.cpu().numpy().view(_lib.REC_FIELDS)[:n]
    pay = t_pay.cpu().numpy()
    for i in range(n):
        assert (pay[pay_off[i] + caps[i]:pay_off[i + 1]] == SENT).all(), "record %d: a byte at or beyond pay_cap" % i
    status, plen = f["status"].astype(np.int64), f["payload_len"].astype(np.int64)
    return status, plen, [pay[o:o + min(int(pl), int(c))].tobytes() for o, pl, c in zip(pay_off[:-1], plen, caps)]


def _guard(k):
    rng = np.random.default_rng(0x6A5D + k)
    data = bytes(np.repeat(rng.integers(0, 256, 40, dtype=np.uint8), rng.integers(1, 30, 40)))
    return dc.Entry("guard", zlib.compress(data, 6), data, 0, "guard")


def _room(e):
    """valid: exactly the bytes; malformed: what the stream produces before its fault, and room to spare (it must never report 5)"""
    return len(e.expected) if e.expected is not None else dc.py_inflate(e.stream, "device").produced + REJECT_ROOM


def _batch(entries, order=None):
    """guard, entry, guard, entry, ..., guard: every entry between two valid streams"""
    ent = list(entries) if order is None else [entries[i] for i in order]
    out = [_guard(0)]
    for k, e in enumerate(ent):
        out += [e, _guard(k + 1)]
    return out


def _check(e, status, plen, got, route, declined=None):
    where = (e.name, route, int(status))
    if route == "par_alone" and status == 8:
        declined.add(e.name)
        return
    if e.expected is not None:
        assert status == 0 and plen == len(e.expected) and got == e.expected, where
    elif e.status is not None:
        assert status == e.status, where
    else:
        assert status not in (0, 5, 6), where


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_catalogue_in_one_batch_in_order_and_shuffled(press, route):
    """the whole catalogue between guard streams through s5gpu_inflate_dev, once in order and once shuffled, on one route per case (the table
    in the module's docstring says which kernels that is; lane_routed tiles the batch to >= 1024 records, and the entries of >= 32 KiB
    are k_inflate_long's).  Valid: status 0, payload_len and bytes exact.  Malformed: the status the catalogue names — the same on every
    full decoder — never 0, 5 or 6, never a byte at or beyond pay_cap.  par_alone: the expected status or 8, and the entries that report 8
    are the ones named in DECLINED_TODAY.
    (lane_routed: when the library finds no scratch for the length-sorted list it launches the unrouted lane kernel instead, silently and
    correctly; nothing a caller can see tells the two apart, so this case cannot prove that k_inflate_simt<true> and k_inflate_long ran.)"""
    cat = dc.catalogue()
    declined = set()
    for order in (None, np.random.default_rng(11).permutation(len(cat))):
        batch = _batch(cat, order)
        if route == "lane_routed":
            batch = batch * (1024 // len(batch) + 1)
            assert len(batch) >= 1024 and sum(len(e.stream) >= 32768 for e in batch) >= 8
        with options(ROUTES[route]):
            status, plen, got = inflate_dev([e.stream for e in batch], [_room(e) for e in batch])
        for e, s, pl, g in zip(batch, status, plen, got):
            _check(e, s, pl, g, route, declined)
    if route == "par_alone":
        assert declined - {"guard"} == DECLINED_TODAY


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_payload_slot_one_byte_too_small(press, route):
    """every valid entry with a slot of one byte less than it needs: status 5 and the exact size (k_inflate, k_inflate_simt<false>, the
    batch tiled to >= 1024 records for k_inflate_simt<true> with k_inflate_long on the entries of >= 32 KiB, and k_inflate_fallback
    behind k_inflate_par, which declines a slot that is too small: 8 with inflate_par = 2), nothing written at or beyond the slot's
    end; the guards between them decode.  (The unpacking k_inflate_par<1> sees too-small slots in
    test_catalogue_through_both_list_shapes_of_the_unpacking_kernel; the host paths size their slots themselves and retry a 5 with the size
    reported, so a caller never sees one: test_host_paths runs them as they are.)"""
    ent = [e for e in dc.catalogue() if e.expected]
    batch = _batch(ent)
    if route == "lane_routed":
        batch = batch * (1024 // len(batch) + 1)
        assert len(batch) >= 1024 and sum(len(e.stream) >= 32768 for e in batch) >= 8
    caps = [len(e.expected) - (1 if e.name != "guard" else 0) for e in batch]
    with options(ROUTES[route]):
        status, plen, got = inflate_dev([e.stream for e in batch], caps)
    for e, s, pl, g in zip(batch, status, plen, got):
        if e.name == "guard":
            assert s == 0 and g == e.expected
        elif route == "par_alone":
            assert s == 8, (e.name, int(s))
        else:
            assert s == 5 and pl == len(e.expected), (e.name, route, int(s), int(pl))


def _solo(streams):
    from slow5tools_amd import _lib
    L = _lib.lib()
    n = len(streams)
    bufs = [C.create_string_buffer(s, max(len(s), 1)) for s in streams]
    inp = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(s) for s in streams])
    out, olen, st = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int32 * n)()
    rc = L.s5gpu_solo_batch(1, n, inp, lens, out, olen, st)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    res = []
    for i in range(n):
        res.append(C.string_at(out[i], olen[i]) if out[i] else None)
        if out[i]:
            libc.free(out[i])
    return rc, res, list(st)


@pytest.mark.gpu
def test_host_paths(press):
    """s5gpu_solo_batch(stage 1) and slow5_ptr_depress_solo(ZLIB): the host sizes every slot from the stream's length and retries a status 5
    with the size reported (k_inflate_par<0> + k_inflate_fallback) — bytes and statuses as on the device routes.  decode_records
    (s5gpu_decode_batch -> s5gpu_decode_dev, k_inflate_par<1>): the catalogue's bytes are no records, so a valid stream reports 0 or 7
    (inflated; what it holds does not parse) and a malformed one the catalogue's status: the inflate's verdict comes first."""
    from slow5tools_amd import _lib
    L = _lib.lib()
    batch = _batch(dc.catalogue())
    rc, res, st = _solo([e.stream for e in batch])
    assert rc == -5
    for e, r, s in zip(batch, res, st):
        _check(e, s, len(r) if r is not None else 0, r, "solo")
        assert (r is None) == (s != 0)
    L.slow5_ptr_depress_solo.restype = C.c_void_p
    L.slow5_ptr_depress_solo.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for e in dc.catalogue():
        cnt = C.c_size_t(12345)
        p = L.slow5_ptr_depress_solo(1, e.stream, len(e.stream), C.byref(cnt))
        if e.expected is None:
            assert not p, e.name
        else:
            assert p and C.string_at(p, cnt.value) == e.expected, e.name
            libc.free(p)
    got = press.decode_records([e.stream for e in batch], raise_on_error=False)
    for e, g in zip(batch, got):
        if e.expected is not None:
            assert g["status"] in (0, 7), (e.name, g["status"])
        elif e.status is not None:
            assert g["status"] == e.status, (e.name, g["status"])
        else:
            assert g["status"] not in (0, 5, 6), (e.name, g["status"])


TOO_SMALL_HERE = ("len_sym_285", "dist_4096", "overlap_d3_o1", "stored_len1_bit3", "final_stored_block_bit5", "match_destination_spans_flush",
                  "more_waiting_matches_than_the_list_holds", "litlen_long_codes_under_many_prefixes", "segments_span_24192")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["list-256", "list-768"])
def test_catalogue_through_both_list_shapes_of_the_unpacking_kernel(press, shape):
    """s5gpu_decode_dev in the full form on the catalogue: k_inflate_par<1, SHORT> (every payload slot <= 32 KiB: the 256-entry waiting list
    and the 7-bit distance table of the svb-zd instantiation; the entries of more than 32 KiB stay out) and k_inflate_par<1, false> (slots
    up to 64 KiB: the 768-entry list), each with k_inflate_fallback and k_unpack_rest behind it.  The catalogue's bytes are no records: a
    valid stream reports 0, 6 or 7 — the unpacker's verdict on what was inflated — with payload_len and the bytes in its slot exact; a
    malformed one reports the inflate's status, which comes first.  The entries of TOO_SMALL_HERE get a slot one byte too small: 5 and the
    exact size (the parallel decoder declines them, k_inflate_fallback names the size), nothing written at or behind the slot's end."""
    from test_svbzd_decode import _dev_decode
    ent = [e for e in dc.catalogue() if shape == "list-768" or _room(e) <= 32768]
    assert {"more_waiting_matches_than_the_list_holds", "dist_4097", "token48_across_the_2048_window", "far_d32506_l3"} <= {e.name for e in ent}
    batch = _batch(ent)
    caps = np.array([_room(e) for e in batch], dtype=np.int64)
    short = {k for k, e in enumerate(batch) if e.name in TOO_SMALL_HERE}
    assert len(short) == len(TOO_SMALL_HERE)
    for k in short:
        caps[k] -= 1
    assert (caps.max() <= 32768) == (shape == "list-256")
    f, _, pay = _dev_decode([e.stream for e in batch], "full", [4096] * len(batch), rec_method=1, pay_caps=caps)
    pay_off = np.concatenate([[0], np.cumsum((caps + 31) // 16 * 16)])
    for k, (e, st, pl, o) in enumerate(zip(batch, f["status"], f["payload_len"], pay_off)):
        if k in short:
            assert st == 5 and pl == len(e.expected), (e.name, shape, int(st), int(pl))
            assert (pay[o + caps[k]:pay_off[k + 1]] == 0).all(), (e.name, shape)          # (_dev_decode's payload buffer starts out zeroed)
        elif e.expected is not None:
            assert st in (0, 6, 7) and pl == len(e.expected) and pay[o:o + pl].tobytes() == e.expected, (e.name, shape, int(st))
        elif e.status is not None:
            assert st == e.status, (e.name, shape, int(st))
        else:
            assert st not in (0, 5, 6), (e.name, shape, int(st))


@functools.lru_cache(maxsize=None)
def _neighbour_cuts():
    """(streams, names): every valid entry of 24 .. 9000 bytes cut at a multiple of 16, and its tail as the next stream.  The cut is the
    first of the multiples of 16, taken in a seeded order, at which running out of input is the first thing wrong (the Python inflate
    under the device's framing says 3; a cut may also leave a wrong code-length sequence in front of the end, which is 2)"""
    rng = np.random.default_rng(16)
    streams, kinds = [], []
    for e in dc.catalogue():
        if e.expected is None or not 24 <= len(e.stream) <= 9000:
            continue
        for c in rng.permutation(np.arange(1, (len(e.stream) - 7) // 16 + 1)):
            cut = 16 * int(c)
            if dc.py_inflate(e.stream[:cut], "device").status == 3:
                streams += [e.stream[:cut], e.stream[cut:]]
                kinds += [e.name, None]
                break
    return streams, kinds


def test_neighbour_cuts_cover_the_catalogue():
    streams, kinds = _neighbour_cuts()
    assert len(streams) >= 150 and all(len(s) % 16 == 0 for s, k in zip(streams, kinds) if k)
    assert all(dc.referee(s) is None for s in streams), ZV


@pytest.mark.gpu
@pytest.mark.parametrize("route", FULL_ROUTES)
def test_truncation_against_the_neighbour(press, route):
    """a stream cut at a multiple of 16 with its own tail as the NEXT record of the batch: the bytes the stream would have continued with
    stand exactly where it would have read them, and a decoder that ignores in_len succeeds.  It must report 3 (the tail, which starts
    in the middle of a stream, must report something other than 0)"""
    streams, kinds = _neighbour_cuts()
    assert len(streams) >= 150
    if route == "lane_routed":
        rep = 1024 // len(streams) + 1
        streams, kinds = streams * rep, kinds * rep
    with options(ROUTES[route]):
        status, plen, got = inflate_dev(streams, [70000 if k else 1024 for k in kinds])
    for k, s in zip(kinds, status):
        if k:
            assert s == 3, (k, route, int(s))
        else:
            assert s != 0


def _head_cases():
    """(entry, cap, bytes of the stream up to and including the token that completes cap)"""
    out = []
    for e in dc.catalogue():
        if not e.expected:
            continue
        marks = dc.py_inflate(e.stream).marks
        for cap in sorted({1, 2, 77, len(e.expected)}):
            if cap <= len(e.expected):
                bit = next(b for b, n in marks if n >= cap)
                out.append((e, cap, 2 + (bit + 7) // 8))
    return out


HEAD_FRONT_FAULTS = ("header_cm_7", "header_cinfo_8", "header_bad_fcheck", "header_fdict", "block_type_3", "stored_nlen_mismatch",
                     "hlit_287", "hlit_288", "hdist_31", "hdist_32", "code_length_code_oversubscribed", "code_length_code_incomplete",
                     "litlen_code_oversubscribed", "litlen_code_incomplete", "litlen_single_code_of_2_bits", "distance_code_oversubscribed",
                     "distance_code_incomplete", "distance_single_code_of_2_bits", "distance_codes_30_of_5_bits", "no_end_of_block_code",
                     "too_far_first_token")


@pytest.mark.gpu
def test_inflate_head(press):
    """s5gpu_inflate_head_dev (k_inflate_head; what slow5_idx_create runs) on every valid entry with pay_cap 1, 2, 77 and the whole
    output: status 0, payload_len = pay_cap (the bytes written), those bytes exact, nothing behind them — given the whole stream, and
    given a front that ends with the byte in which the token that completes pay_cap ends (a stored block counts as one token: its
    bytes are copied as a block).  A front one byte shorter reports 3.
    Malformed entries: the ones whose fault stands in front of the first byte of output (HEAD_FRONT_FAULTS: wrapper, block type, NLEN,
    HLIT / HDIST, every wrong code set, a match as the first token) report the catalogue's status with pay_cap 1, given the whole stream;
    and a front of too_far_first_token that ends inside that token reports 3, not 2 (the token ran over the end of the input: the cut's
    doing, whatever the zero bits behind it make of it).  The other malformed entries are not held to a status here: this entry point
    reads no further than the head and no trailer, so a fault behind the head — or in where the data ends — is not its business."""
    cases = _head_cases()
    assert len(cases) > 500
    streams = [e.stream for e, _, _ in cases]
    caps = [c for _, c, _ in cases]
    for what, in_lens, want in (("whole", None, 0), ("front", [n for _, _, n in cases], 0), ("short front", [n - 1 for _, _, n in cases], 3)):
        status, plen, got = inflate_dev(streams, caps, head=True, in_lens=in_lens)
        for (e, cap, n), s, pl, g in zip(cases, status, plen, got):
            assert s == want, (e.name, cap, what, int(s))
            if want == 0:
                assert pl == cap and g == e.expected[:cap], (e.name, cap, what)
    cat = dc.by_name()
    bad = [cat[n] for n in HEAD_FRONT_FAULTS]
    assert all(e.expected is None and e.status in (1, 2) and dc.py_inflate(e.stream, "device").produced == 0 for e in bad)
    streams = [e.stream for e in bad] + [cat["too_far_first_token"].stream]
    status, plen, _ = inflate_dev(streams, [1] * len(streams), head=True, in_lens=[len(e.stream) for e in bad] + [3])
    for e, s in zip(bad, status):
        assert s == e.status, (e.name, int(s))
    assert status[-1] == 3 and (plen == 0).all()


# ---------------------------------------------------------------- record payloads in crafted blocks
HDR_ARGS = (8192.0, 23.0, 1467.61, 4000.0)


def runs_as_tokens(p):
    """literals, and a distance-1 match for every run of five or more equal bytes"""
    toks, i, n = [], 0, len(p)
    while i < n:
        j = i
        while j < n and p[j] == p[i]:
            j += 1
        toks.append(dc.lit(p[i]))
        run = j - i - 1
        while run >= 4:
            m = min(run, 258)
            if run - m in (1, 2, 3):
                m -= 3
            toks.append(dc.match(m, 1))
            run -= m
        toks += [dc.lit(p[i])] * run
        i = j
    return toks


def far_tokens(p, least=700):
    """literals, and a match of 3 .. 258 bytes wherever the next three bytes also stand at least `least` bytes back"""
    first, toks, i, n = {}, [], 0, len(p)
    while i < n:
        at = first.get(p[i:i + 3]) if i + 3 <= n else None
        if at is not None and i - at >= least:
            m = 3
            while m < 258 and i + m < n and p[at + m] == p[i + m]:
                m += 1
            toks.append(dc.match(m, i - at))
            step = m
        else:
            toks.append(dc.lit(p[i]))
            step = 1
        for k in range(i, i + step):
            first.setdefault(p[k:k + 3], k)
        i += step
    return toks


def record_streams(p):
    """{shape: stream} of one record payload"""
    cuts = [0, 1, 8, 71, 1000]
    pieces = [p[a:b] for a, b in zip(cuts, cuts[1:] + [len(p)]) if a < len(p)] or [b""]
    out = {}
    st = dc.Stream()
    for k, x in enumerate(pieces):
        st.stored(x, final=k == len(pieces) - 1)
    out["stored_splits_in_the_head"] = st
    out["fixed_literals"] = dc.Stream().fixed(dc.lits(p), final=True)
    out["fixed_runs"] = dc.Stream().fixed(runs_as_tokens(p), final=True)
    out["dynamic_far_matches"] = dc.Stream().dynamic(far_tokens(p), dc.FLAT286, dc.DIST30, final=True)
    st = dc.Stream()
    step = max(1, (len(p) + 39) // 40)
    for k in range(40):
        x = p[k * step:(k + 1) * step]
        if k % 3 == 0:
            st.fixed(dc.lits(x), final=k == 39)
        elif k % 3 == 1:
            st.stored(x, final=k == 39)
        else:
            st.dynamic(dc.lits(x), dc.FLAT286, [0], final=k == 39)
    out["forty_tiny_blocks"] = st
    for st in out.values():
        assert st.valid and bytes(st.out) == p
    return {k: st.zlib() for k, st in out.items()}


def test_record_shapes_hold_the_payload():
    rng = np.random.default_rng(4)
    for n in (0, 1, 50, 3000):
        p = bytes(np.repeat(rng.integers(0, 8, n // 3 + 1, dtype=np.uint8), rng.integers(1, 9, n // 3 + 1))[:n])
        for shape, s in record_streams(p).items():
            assert dc.referee(s) == p and dc.py_inflate(s).data == p, (shape, n, ZV)
    assert any(t[0] == "match" and t[2] >= 700 for t in far_tokens(bytes(rng.integers(0, 4, 3000, dtype=np.uint8))))


def _records(press, sm):
    """[(shape, stream, payload, signal, aux, index)] of reads of 0, 1, 1500 and 4000 samples with aux bytes"""
    rng = np.random.default_rng(61)
    sigs = [(500 + np.cumsum(rng.integers(-15, 16, n)) % 300).astype(np.int16) for n in (0, 1, 1500, 4000)]
    sigs.append(np.repeat(rng.integers(300, 700, 100), rng.integers(1, 80, 100))[:4000].astype(np.int16))        # plateaus: runs in the payload
    hdrs = [press.pack_hdr(b"read_%06d" % i, i % 3, *HDR_ARGS) for i in range(len(sigs))]
    auxs = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in (0, 3, 40, 17, 9)]
    raw = press.encode_records(sigs, hdrs, auxs, press.REC_NONE, sm)
    out = []
    for i, r in enumerate(raw):
        for shape, s in record_streams(r[8:]).items():
            out.append((shape, s, r[8:], sigs[i], auxs[i], i))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("sig_name", ["svb-zd", "ex-zd"])
def test_record_payloads_in_crafted_blocks(press, sig_name):
    """real record payloads (zlib + svb-zd, zlib + ex-zd; 0, 1, 1500 and 4000 samples, with aux bytes) written as stored splits in the
    head, fixed blocks of literals and of runs, a dynamic block with far matches, and forty tiny blocks of all three kinds, through
      * decode_records with unpack_fused 1 and 0: s5gpu_decode_dev in the full form — k_inflate_par<1 | 2, SHORT> + k_inflate_fallback +
        k_unpack_rest, and k_inflate_par<0> + k_unpack; and with payload slots of 40 000 bytes the 768-entry list shape (k_inflate_par<.., false>)
      * S5GPU_DEC_NO_PAYLOAD with max_in_len <= 4000 on the records of one window: k_inflate_par_np_lp keeps a one-block Huffman record in
        LDS and declines the stored and the multi-block shapes, which k_inflate_fallback_np redoes in its scratch slot
      * S5GPU_DEC_NO_PAYLOAD with max_in_len unknown: k_inflate_par_np + k_inflate_fallback_np
    signals and fields exact everywhere"""
    from slow5tools_amd import _lib
    from test_svbzd_decode import _dev_decode
    sm = {"svb-zd": press.SIG_SVB_ZD, "ex-zd": press.SIG_EX_ZD}[sig_name]
    recs = _records(press, sm)
    assert len(recs) >= 12
    streams = [s for _, s, _, _, _, _ in recs]
    for fused in (1, 0):
        with options({b"unpack_fused": fused}):
            got = press.decode_records(streams, press.REC_ZLIB, sm)
        for (shape, _, pay, sig, aux, i), g in zip(recs, got):
            assert g["status"] == 0 and np.array_equal(g["signal"], sig) and g["aux"] == aux and g["payload"] == pay, (shape, i, fused)
            assert g["read_id"] == b"read_%06d" % i and g["read_group"] == i % 3

    def check(f, sig_out, which):
        for (shape, _, pay, sig, aux, i), k in zip(recs, range(len(recs))):
            if k in which:
                j = which.index(k)
                assert f["status"][j] == 0 and np.array_equal(sig_out[j], sig), (shape, i, int(f["status"][j]))
                assert f["n_samples"][j] == len(sig) and f["aux_len"][j] == len(aux) and f["read_group"][j] == i % 3 and f["read_id_len"][j] == 11

    every = list(range(len(recs)))
    caps = [len(sig) for _, _, _, sig, _, _ in recs]
    f, so, _ = _dev_decode(streams, "full", caps, rec_method=1, pay_caps=[40000] * len(recs), sig_method=sm)
    check(f, so, every)
    f, so, _ = _dev_decode(streams, "np", caps, rec_method=1, np_cap=max(len(p) for _, _, p, _, _, _ in recs) + 64, sig_method=sm)
    check(f, so, every)
    short = [k for k, (_, s, p, _, _, _) in enumerate(recs) if len(s) <= 3900 and len(p) <= 3600]
    assert len(short) >= 8 and {recs[k][0] for k in short} == set(record_streams(b"x"))
    f, so, _ = _dev_decode([streams[k] for k in short], "np", [caps[k] for k in short], rec_method=1, np_cap=5344, max_in_len=4000, sig_method=sm)
    check(f, so, short)
    assert _lib.DEC_NO_PAYLOAD == 1


# ---------------------------------------------------------------- mutants on the device
@pytest.mark.gpu
@pytest.mark.parametrize("route", FULL_ROUTES)
def test_mutants_against_stock_zlib(press, route):
    """600 seeded mutants of the valid catalogue streams, stock zlib refereeing both ways on every full route: what the device accepts
    zlib accepts, with the same bytes; what zlib accepts the device accepts"""
    M, ref = mutants(), mutant_answers()
    keep = [k for k, (_, g) in enumerate(M) if not excluded(g)]
    streams = [M[k][1] for k in keep]
    caps = [len(ref[k]) if ref[k] is not None else 1 << 17 for k in keep]
    if route == "lane_routed":
        streams, caps, keep = streams * 2, caps * 2, keep * 2
    with options(ROUTES[route]):
        status, plen, got = inflate_dev(streams, caps)
    for k, s, pl, g in zip(keep, status, plen, got):
        if s == 0:
            assert ref[k] is not None and g == ref[k], (M[k][0], k, route, ZV)
        else:
            assert ref[k] is None, (M[k][0], k, route, int(s), ZV)
