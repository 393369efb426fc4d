"""ex-zd decoders on hand-made blobs: every device route against a plain numpy / Python-integer reference, valid and malformed.

The encoders (ours and the oracle's) only ever write minimal StreamVByte widths, the canonical q, increasing exception positions
and section lengths that match their contents.  The format allows more — widths wider than needed, any q up to 15, values that
wrap 32 bits — and a decoder has to refuse a blob that does not add up (status 7, as oracle/exzd.c refuses it).  The blobs below
are written field by field by `exzd_blob`, independent of any encoder, decoded by `ref_decode`, and refereed by the oracle
(`s5o_exzd_decode`, called with a small buffer: it rejects every malformed entry before its first store).

Entries that pin the three prologue / chunk rules of the device decoders (exzd_decode_wg, exzd_decode_wave), with what the decoders
gave before those rules:
  * count_fffffff0_L26, count_2p30_L64, count_2L_plus_65: a count the blob cannot hold (every position costs at least one byte:
    N - 1 <= L - 16).  Every device call answered 6 ("signal slot too small", n_samples up to 4.29 G); the host batches retried
    with a slot of that size and only then arrived at 7.  It must be 7 at once.
  * gap_fffffffd (both decoders) and backstep_chunk512 (the workgroup decoder, where entry 511 sits inside a chunk): exception
    positions summed in 32 bits, so a huge gap is a step backwards; a distinct position inside the same tile passed every later
    check and the values were handed out by rank, not in list order: status 0 with samples no reference decoder produces.
    gap_ffffffff, backstep_chunk4096, wrapped_sum_in_chunk and backstep_chunk512 on the wave decoder were refused already, by the
    later checks (a position used twice, the tile that cannot advance, an entry no tile reaches).
  * slack_pos, slack_val: a section longer than the keys and data it holds: status 0 on every route.
"""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import oracle_bind as ob
import test_svbzd_decode as sv
from signal_craft import M32, WIDTH_END, WIDTH_LO, _balance, _decode, _gaps, _min_codes, _svb32_read, exzd_blob, fields, svb32   # noqa: F401  (the builders: tests/signal_craft.py)
from signal_craft import exzd_ref_decode as ref_decode
from test_svbzd_decode import RUN_AUX, SENT, _aux, _interleave, _np_cap, _opt, press   # noqa: F401  (press: the fixture)

HDR_ARGS = sv.HDR_ARGS
SIG_EX_ZD = 2


def _full_width(rng, codes, top=1 << 31):
    """a value for every code that needs all of its bytes (any byte for code 0), below top"""
    codes = np.asarray(codes, dtype=np.int64)
    lo = np.array(WIDTH_LO, dtype=np.float64)[codes]
    hi = np.minimum(np.array(WIDTH_END, dtype=np.float64)[codes], top)
    return np.minimum(lo + np.floor(rng.random(len(codes)) * (hi - lo)), hi - 1).astype(np.uint64)


def _vals(rng, k):
    """small exception values: deltas of a few hundred, signs balanced"""
    return _balance(rng.integers(0, 1200, k).astype(np.uint64))


def _rest(rng, k):
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes()      # random bytes, not runs: zlib streams of them stay in the parallel inflate


def _make(rng, N, pos, vals=None, q=0, z0=None, **kw):
    """a blob of N samples with exceptions on the given (increasing) positions; everything not given is random"""
    pos = np.asarray(pos, dtype=np.int64)
    vals = _vals(rng, len(pos)) if vals is None else vals
    z0 = int(rng.integers(0, 4000)) if z0 is None else z0
    return exzd_blob(N, q, z0, _gaps(pos), vals, _rest(rng, N - 1 - len(pos)), **kw)


def _pick(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), k, replace=False))


NEX_COUNTS = (511, 512, 513, 1024, 4095, 4096, 4097, 8192)
LAST_TILE = (1, 15, 16, 17)
BAD_COUNT = ("count_fffffff0_L26", "count_2p30_L64", "count_L_minus_14", "count_2L_plus_65")


def _patch(blob, off, fmt, v):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, v)
    return bytes(b)


def _backstep(rng, chunk, N, nex):
    """(bad, mended) gaps: entry chunk - 1, the last of the first exception chunk, steps two positions back onto a free position
    (gap 0xFFFFFFFD in 32 bits), and more entries follow it; mended has gap 0 there"""
    g = rng.integers(0, max(1, (N - 40) // nex - 1), nex).astype(np.int64)
    g[chunk - 2] = 4
    g[chunk] = 6
    bad = g.copy()
    bad[chunk - 1] = 0xFFFFFFFD
    g[chunk - 1] = 0
    assert int((g + 1).sum()) < N - 1
    return bad, g


def _corpus():
    """([(name, blob)], {malformed name: the blob with only the stated defect undone}): valid small blobs, malformed ones, then
    the long valid ones (so every malformed blob has long records behind it in a batch)"""
    rng = np.random.default_rng(0xE72D)
    small, bad, big, mended = [], [], [], {}

    def malformed(name, blob, fix):
        bad.append((name, blob))
        mended[name] = fix

    # ---- valid: sizes, counts
    small.append(("n0", exzd_blob(0, 0, 0, [], [], b"")))
    small.append(("n1", exzd_blob(1, 0, 77, [], [], b"")))
    small.append(("n2_plain", exzd_blob(2, 0, 5, [], [], b"\x09")))
    small.append(("n2_exception", exzd_blob(2, 0, 5, [0], [700], b"")))
    small.append(("n17", _make(rng, 17, [4])))                                             # sixteen positions: one lane exactly
    small.append(("nex0_n3000", _make(rng, 3000, [])))
    small.append(("all_exceptions_n600", _make(rng, 600, np.arange(599))))                 # nex = N - 1: no rest bytes at all
    # ---- valid: positions
    small.append(("pos_0_and_last", _make(rng, 5000, [0, 4998])))
    small.append(("lane_neighbours", _make(rng, 3000, [21, 79, 80, 1024 + 48 + 15, 2048 + 64])))   # sixteen free positions next to a lane with one
    # ---- valid: values and q
    # y0 = 1000; -2^31 (0xFFFFFEFF), +2^31 - 1, +128 (val 0, z = 256), -128 (0xFFFFFFFF: z wraps to 255), then +-40000: out of int16 and back
    small.append(("extreme_values", exzd_blob(200, 0, 2000, _gaps([0, 1, 2, 3, 50, 51, 120, 121]),
                                              [0xFFFFFEFF, 0xFFFFFEFE, 0, 0xFFFFFFFF, 79744, 79743, 79999 - 256, 80000 - 256], _rest(rng, 191))))
    small.append(("small_values_in_four_bytes", _make(rng, 2000, _pick(rng, 0, 1999, 400), vals=_balance(rng.integers(0, 200, 400)),
                                                      gap_codes=np.full(400, 3), val_codes=np.full(400, 3))))
    pos = _pick(rng, 0, 2999, 500)
    small.append(("non_minimal_widths", _make(rng, 3000, pos, gap_codes=np.maximum(_min_codes(_gaps(pos)), rng.integers(0, 4, 500)),
                                              val_codes=np.maximum(1, rng.integers(0, 4, 500)))))
    even = np.array([0, 3], dtype=np.uint8)[rng.integers(0, 2, 1490)] + 4 * rng.integers(0, 64, 1490).astype(np.uint8)   # z % 4 in {0, 3}: even deltas
    small.append(("q0_all_even", exzd_blob(1500, 0, 2 * 600, _gaps([7, 8, 100, 700, 701, 702, 1200, 1300, 1498]),
                                           [4 * 100, 4 * 100 + 3, 4 * 90, 4 * 90 + 3, 0, 3, 4, 7, 8], even.tobytes())))
    small.append(("q15", _make(rng, 1000, _pick(rng, 0, 999, 30), q=15)))
    small.append(("q7_drops_set_bits", _make(rng, 1100, _pick(rng, 0, 1099, 30), q=7)))
    x = (4 * rng.integers(-2000, 2000, 900)).astype(np.int16)                              # canonical q = 2 (or more), written with q = 1
    small.append(("q_below_canonical", exzd_blob(*fields(x, 1))))
    small.append(("z0_ffff", _make(rng, 300, [5, 200], z0=0xFFFF)))

    # ---- malformed
    good_pos = _pick(rng, 0, 1499, 20)
    good_vals = _vals(rng, 20)
    good_rest = _rest(rng, 1479)
    good = exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest)
    o_plen = 16                                                                            # u32 len of the position section
    o_vlen = 20 + struct.unpack_from("<I", good, o_plen)[0]
    assert ref_decode(good) is not None
    for L in range(16):
        malformed("L%d" % L, good[:L], good)
    malformed("n0_L11", exzd_blob(0, 0, 0, [], [], b"") + b"\x00", exzd_blob(0, 0, 0, [], [], b""))
    malformed("version_1", exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest, version=1), good)
    malformed("q_16", exzd_blob(1500, 16, 300, _gaps(good_pos), good_vals, good_rest), good)
    malformed("count_fffffff1", _patch(good, 1, "<Q", 0xFFFFFFF1), good)
    for name, N, L in (("count_fffffff0_L26", 0xFFFFFFF0, 26), ("count_2p30_L64", 1 << 30, 64), ("count_L_minus_14", 40 - 14, 40),
                       ("count_2L_plus_65", 2 * 40 + 65, 40)):
        r = _rest(rng, L - 16)
        malformed(name, exzd_blob(N, 0, 9, [], [], r), exzd_blob(L - 15, 0, 9, [], [], r))
    malformed("nex_is_N", exzd_blob(5, 0, 9, [0, 0, 0, 0], [1, 2, 3, 4], b"", nex=5), exzd_blob(5, 0, 9, [0, 0, 0, 0], [1, 2, 3, 4], b""))
    malformed("nex_above_lists", exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest, nex=21), good)
    malformed("nex_below_lists", exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest, nex=19), good)
    malformed("section_len_below_keys", _patch(good, o_plen, "<I", 4), good)               # 20 entries: 5 key bytes
    malformed("section_len_beyond_L", _patch(good, o_vlen, "<I", len(good)), good)
    malformed("slack_pos", exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest, slack=(b"\x00", b"")), good)
    malformed("slack_val", exzd_blob(1500, 0, 300, _gaps(good_pos), good_vals, good_rest, slack=(b"", b"\x00")), good)
    # the last data byte of the position section gone, its length one less: the last gap reads past the section
    short = _patch(good[:o_vlen - 1] + good[o_vlen:], o_plen, "<I", struct.unpack_from("<I", good, o_plen)[0] - 1)
    malformed("section_data_one_short", short, good)
    # one data byte per entry, but the keys of the first exception chunk claim four: the data runs out in that chunk
    for chunk, N, nex in ((512, 6000, 1200), (4096, 12500, 9000)):
        pos = _pick(rng, 0, N - 1, nex)
        g = np.minimum(_gaps(pos), 255)
        g[0] = 0
        pos = np.cumsum(g + 1) - 1
        fix = exzd_blob(N, 0, 40, g, rng.integers(0, 256, nex), _rest(rng, N - 1 - nex))
        malformed("overclaim_first_chunk_%d" % chunk, fix[:20] + b"\xFF" * (chunk // 4) + fix[20 + chunk // 4:], fix)
    malformed("rest_one_more", good + b"\x21", good)
    malformed("rest_one_less", good[:-1], good)
    malformed("last_position_is_N_minus_1", exzd_blob(100, 0, 8, _gaps([10, 99]), [5, 6], _rest(rng, 97)),
              exzd_blob(100, 0, 8, _gaps([10, 98]), [5, 6], _rest(rng, 97)))
    r97 = _rest(rng, 97)
    malformed("gap_ffffffff", exzd_blob(100, 0, 8, [10, 0xFFFFFFFF], [300, 900], r97), exzd_blob(100, 0, 8, [10, 1], [300, 900], r97))
    malformed("gap_fffffffd", exzd_blob(100, 0, 8, [10, 0xFFFFFFFD], [300, 900], r97), exzd_blob(100, 0, 8, [10, 1], [300, 900], r97))
    for chunk, N, nex in ((512, 4000, 600), (4096, 12800, 4200)):
        b_, g_ = _backstep(rng, chunk, N, nex)
        v, r = _vals(rng, nex), _rest(rng, N - 1 - nex)
        malformed("backstep_chunk%d" % chunk, exzd_blob(N, 0, 8, b_, v, r), exzd_blob(N, 0, 8, g_, v, r))
    # 5, then 2^31 + 6 (far outside), then 2^32 + 8: in 32 bits the chunk's last positions are back inside the signal
    g = np.concatenate([[5, 0x80000000, 0x80000001], rng.integers(0, 9, 37)]).astype(np.int64)
    v, r = _vals(rng, 40), _rest(rng, 959)
    g_ = g.copy()
    g_[1:3] = (1, 0)
    malformed("wrapped_sum_in_chunk", exzd_blob(1000, 0, 8, g, v, r), exzd_blob(1000, 0, 8, g_, v, r))

    # ---- valid, long
    for k in NEX_COUNTS:
        N = {4095: 9000, 4096: 9001, 4097: 9002, 8192: 12500}.get(k, 3 * k)
        big.append(("nex%d" % k, _make(rng, N, _pick(rng, 0, N - 1, k))))
    big.append(("pos_tile_edges", _make(rng, 9000, [1023, 1024, 4095, 4096])))
    # the last entry of the first exception chunk sits mid-tile, the next chunk's first entry right behind it (gap 0)
    big.append(("chunk_cut_512", _make(rng, 6000, np.concatenate([_pick(rng, 0, 1400, 511), [1500, 1501], _pick(rng, 1502, 5999, 100)]))))
    big.append(("chunk_cut_4096", _make(rng, 12800, np.concatenate([_pick(rng, 0, 6000, 4095), [6100, 6101], _pick(rng, 6102, 12799, 200)]))))
    big.append(("isolated_far_apart", _make(rng, 12900, [100, 4300, 8500, 12700])))
    for t in LAST_TILE:                                                                    # 4096 = 4 x 1024: the last tile of both decoders
        big.append(("last_tile_%d" % t, _make(rng, 4097 + t, [3, 1000, 4090, 4096])))
    # gaps: any byte is a full-width code 0 (kept below 8 here, for the size), a dozen two-byte ones; values: codes 0-3, every byte needed
    k = 1200
    gc = np.zeros(k, dtype=np.int64)
    gc[_pick(rng, 1, k, 12)] = 1
    g = np.where(gc == 1, _full_width(rng, gc, top=1 << 9), rng.integers(0, 8, k).astype(np.uint64))
    pos = np.cumsum(g.astype(np.int64) + 1) - 1
    vc = rng.integers(0, 4, k)
    N = int(pos[-1]) + 40
    assert N < 13000
    big.append(("random_codes_full_width", exzd_blob(N, 0, 11, g, _balance(_full_width(rng, vc, top=1 << 30)), _rest(rng, N - 1 - k),
                                                     gap_codes=gc, val_codes=vc)))
    big.append(("gap_needs_three_bytes", _make(rng, 70001, [5, 5 + 1 + 66000, 66010, 69990])))
    return small + bad + big, mended


CORPUS, MENDED = _corpus()
REF = {name: ref_decode(blob) for name, blob in CORPUS}
MALFORMED = {name for name, _ in CORPUS if REF[name] is None}


def _guards(k):
    """valid, short blobs that sit between the corpus entries of a batch"""
    rng = np.random.default_rng(0x6A5E + k)
    out = []
    for _ in range(k):
        N = int(rng.integers(200, 900))
        out.append(_make(rng, N, _pick(rng, 0, N - 1, int(rng.integers(0, 12)))))
    return out


# ---------------------------------------------------------------- CPU: the reference against the oracle

def test_corpus_has_every_promised_shape():
    names = {n for n, _ in CORPUS}
    assert len(names) == len(CORPUS)
    valid = names - MALFORMED
    assert {"n0", "n1", "n2_plain", "n2_exception", "n17", "nex0_n3000", "all_exceptions_n600", "pos_0_and_last", "lane_neighbours", "extreme_values",
            "small_values_in_four_bytes", "non_minimal_widths", "q0_all_even", "q15", "q7_drops_set_bits", "q_below_canonical", "z0_ffff",
            "pos_tile_edges", "chunk_cut_512", "chunk_cut_4096", "isolated_far_apart", "random_codes_full_width",
            "gap_needs_three_bytes"} | {"nex%d" % k for k in NEX_COUNTS} | {"last_tile_%d" % t for t in LAST_TILE} == valid
    assert MALFORMED == set(MENDED) and MALFORMED >= {"L%d" % L for L in range(16)} | set(BAD_COUNT) | {
        "n0_L11", "version_1", "q_16", "count_fffffff1", "nex_is_N", "nex_above_lists", "nex_below_lists", "section_len_below_keys",
        "section_len_beyond_L", "slack_pos", "slack_val", "section_data_one_short", "overclaim_first_chunk_512", "overclaim_first_chunk_4096",
        "rest_one_more", "rest_one_less", "last_position_is_N_minus_1", "gap_ffffffff", "gap_fffffffd", "backstep_chunk512",
        "backstep_chunk4096", "wrapped_sum_in_chunk"}
    blobs = dict(CORPUS)
    assert len(blobs["n0"]) == 10 and len(blobs["n1"]) == 16 and len(blobs["count_fffffff0_L26"]) == 26
    # each malformed entry is malformed for its stated reason only: with that one defect undone it decodes
    for name in MALFORMED:
        assert ref_decode(MENDED[name]) is not None, name
    # a count the blob cannot hold, and nothing else wrong with the header
    for name in BAD_COUNT:
        b = blobs[name]
        N, = struct.unpack_from("<Q", b, 1)
        assert 0 < N <= 0xFFFFFFF0 and N - 1 > len(b) - 16 and struct.unpack_from("<I", b, 12)[0] == 0, name
    # the oracle accumulates y in int32: every valid entry stays inside it
    for name in valid:
        assert _decode(blobs[name])[1] < 2**31 - 1, name
    sizes = {n: len(REF[n]) for n in valid}
    assert max(sizes.values()) == sizes["gap_needs_three_bytes"] == 70001 and sorted(sizes.values())[-2] < 13000
    # shapes that the names promise
    assert struct.unpack_from("<I", blobs["all_exceptions_n600"], 12)[0] == 599 and struct.unpack_from("<I", blobs["nex0_n3000"], 12)[0] == 0
    assert blobs["q15"][9] == 15 and blobs["q0_all_even"][9] == 0 and not (REF["q0_all_even"] & 1).any()
    assert blobs["q_below_canonical"][9] == 1 < fields(REF["q_below_canonical"])[1]
    assert blobs["q7_drops_set_bits"][9] == 7 and _decode(blobs["q7_drops_set_bits"])[1] >= 1 << 9   # set bits of y beyond 16 - q are dropped
    assert int.from_bytes(blobs["z0_ffff"][10:12], "little") == 0xFFFF and REF["z0_ffff"][0] == -32768
    ev = REF["extreme_values"].astype(np.int64)
    assert int(ev[51]) - int(ev[50]) == 40000 - 65536 and ev[52] == ev[50]                   # a step that leaves int16, and comes back
    # the two back steps land on a free position inside the first chunk's reach, and entries follow
    for chunk, name in ((512, "backstep_chunk512"), (4096, "backstep_chunk4096")):
        b = blobs[name]
        nex, = struct.unpack_from("<I", b, 12)
        g = _svb32_read(b[20:20 + struct.unpack_from("<I", b, 16)[0]], nex)
        p = (np.cumsum(g + 1) - 1) & M32
        assert nex > chunk and p[chunk - 1] == p[chunk - 2] - 2 and len(set(p.tolist())) == nex and p.max() < struct.unpack_from("<Q", b, 1)[0] - 1
    # the overclaiming blobs carry one data byte per entry: their count and section lengths fit, only the key claims do not
    for chunk in (512, 4096):
        b = blobs["overclaim_first_chunk_%d" % chunk]
        nex, sl = struct.unpack_from("<II", b, 12)
        assert sl == (nex + 3) // 4 + nex and nex > chunk and b[20:20 + chunk // 4] == b"\xFF" * (chunk // 4)


def oracle_decode(blob):
    return ob.exzd_decode_bounded(blob)


@pytest.mark.parametrize("name", [n for n, _ in CORPUS])
def test_reference_equals_the_oracle(name):
    blob = dict(CORPUS)[name]
    want, got = REF[name], oracle_decode(blob)
    if want is None:
        assert got is None, name
    else:
        assert got is not None and np.array_equal(got, want), name
        # and the other way round: the oracle's encoding of those samples decodes to them
        enc = ob.exzd_encode(want)
        assert np.array_equal(ref_decode(enc), want) and np.array_equal(oracle_decode(enc), want)


def test_builder_fed_the_canonical_choice_is_the_encoder():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 5, 1000, 4098):
        for x in (rng.integers(-32768, 32768, n).astype(np.int16), (8 * rng.integers(-3000, 3000, n)).astype(np.int16),
                  (500 + rng.integers(-40, 40, n)).astype(np.int16)):
            blob = exzd_blob(*fields(x))
            assert blob == ob.exzd_encode(x), n
            assert np.array_equal(ref_decode(blob), x)


def test_guards_are_valid():
    for g in _guards(8):
        assert ref_decode(g) is not None and oracle_decode(g) is not None


# ---------------------------------------------------------------- GPU routes

def _payload(blob, i):
    from slow5tools_amd import press as p
    return p.pack_hdr(b"rd%d" % i, i, *HDR_ARGS) + struct.pack("<Q", len(blob)) + blob + _aux(i)


def _check(name, status, n_samples, signal, aux=None, want_aux=None):
    """a valid entry: status 0 and exact samples; a malformed one: status 7, on every route"""
    want = REF[name] if isinstance(name, str) else name
    if want is None:
        assert status == 7, (name, status)
    else:
        assert status == 0, (name, status)
        assert n_samples == len(want) and np.array_equal(signal, want), name
        if want_aux is not None:
            assert aux == want_aux, name


def _batch(keep=None):
    """(names, blobs): the corpus between guards; names of guards are their reference signals"""
    items = [(n, b) for n, b in CORPUS if keep is None or n in keep]
    g = _guards(len(items) + 1)
    blobs = _interleave([b for _, b in items], g)
    names = _interleave([n for n, _ in items], [ref_decode(x) for x in g])
    return names, blobs


def _sig_caps(names, blobs):
    """valid: exactly the samples; malformed: the blob's byte count (what a caller sizing by the blob would give: a count the blob
    cannot hold does not fit it, and must still be 7, never 6)"""
    return [len(REF[nm] if isinstance(nm, str) else nm) if (not isinstance(nm, str) or REF[nm] is not None) else len(b)
            for nm, b in zip(names, blobs)]


def _dev(recs, form, caps, **kw):
    return sv._dev_decode(recs, form, caps, sig_method=SIG_EX_ZD, **kw)


def _check_dev(names, f, sig):
    for i, nm in enumerate(names):
        _check(nm, int(f["status"][i]), int(f["n_samples"][i]), sig[i])
        if f["status"][i] == 0:
            assert f["aux_len"][i] == 3 and f["read_group"][i] == i


def _check_host(names, recs_out, pays=None):
    for i, (nm, g) in enumerate(zip(names, recs_out)):
        _check(nm, g["status"], len(g.get("signal", ())), g.get("signal"), g.get("aux"), _aux(i))
        if g["status"] == 0:
            assert g["read_group"] == i and g["read_id"] == b"rd%d" % i
            if pays is not None:
                assert g["payload"] == pays[i]


@pytest.fixture(scope="module")
def batch():
    names, blobs = _batch()
    pays = [_payload(b, i) for i, b in enumerate(blobs)]
    return names, blobs, pays, [zlib.compress(p, 6) for p in pays]


@pytest.mark.gpu
def test_workgroup_decoder_without_record_press(press, batch):
    """k_unpack -> exzd_decode_wg: records without a record press, through the host batch (which sizes the slots itself and retries
    a status 6) and through one device call with the slots of _sig_caps"""
    names, blobs, pays, _ = batch
    _check_host(names, press.decode_records(pays, press.REC_NONE, press.SIG_EX_ZD, raise_on_error=False), pays)
    f, sig, _ = _dev(pays, "full", _sig_caps(names, blobs), rec_method=0, pay_caps=[len(p) + 64 for p in pays])
    _check_dev(names, f, sig)


@pytest.mark.gpu
def test_workgroup_decoder_behind_the_inflate(press, batch):
    """zlib records with unpack_fused = 0: k_inflate_par<0> / fallback, then k_unpack -> exzd_decode_wg"""
    names, blobs, pays, streams = batch
    _opt(b"unpack_fused", 0)
    try:
        _check_host(names, press.decode_records(streams, press.REC_ZLIB, press.SIG_EX_ZD, raise_on_error=False), pays)
        f, sig, _ = _dev(streams, "full", _sig_caps(names, blobs), rec_method=1, pay_caps=[len(p) + 64 for p in pays])
    finally:
        _opt(b"unpack_fused", 1)
    _check_dev(names, f, sig)


@pytest.mark.gpu
def test_wave_decoder_behind_the_parallel_inflate(press, batch):
    """k_inflate_par<2> -> exzd_decode_wave: zlib records, default options — the wave that inflates a record decodes its blob.  That
    the parallel decoder takes every one of these records: with inflate_par = 2 (no fallback pass) none reports 8."""
    names, blobs, pays, streams = batch
    _check_host(names, press.decode_records(streams, press.REC_ZLIB, press.SIG_EX_ZD, raise_on_error=False), pays)
    f, sig, _ = _dev(streams, "full", _sig_caps(names, blobs), rec_method=1, pay_caps=[len(p) + 64 for p in pays])
    _check_dev(names, f, sig)
    _opt(b"inflate_par", 2)
    try:
        alone = press.decode_records(streams, press.REC_ZLIB, press.SIG_EX_ZD, raise_on_error=False)
    finally:
        _opt(b"inflate_par", 1)
    assert not [i for i, g in enumerate(alone) if g["status"] == 8]
    _check_host(names, alone, pays)


FALLBACK_VALID = ("n0", "n17", "last_tile_1", "nex4097", "non_minimal_widths", "q15")    # N = 0, 17, 4098, ...


@pytest.mark.gpu
def test_fallback_inflate_then_unpack_rest(press):
    """k_inflate_fallback + k_unpack_rest -> exzd_decode_wg: the malformed entries and six valid ones, each record with a long run
    of zeros in its aux field (declined by the parallel decoder: inflate_par = 2 leaves status 8 on each), between short guards
    that the parallel decoder takes and decodes itself — k_unpack_rest must pick exactly the others"""
    assert len(REF["last_tile_1"]) == 4098
    names, blobs = _batch(MALFORMED | set(FALLBACK_VALID))
    pays = []
    for i, (nm, b) in enumerate(zip(names, blobs)):
        p = _payload(b, i)
        pays.append(p + RUN_AUX if isinstance(nm, str) else p)
    streams = [zlib.compress(p, 6) for p in pays]
    got = press.decode_records(streams, press.REC_ZLIB, press.SIG_EX_ZD, raise_on_error=False)
    for i, (nm, r) in enumerate(zip(names, got)):
        _check(nm, r["status"], len(r.get("signal", ())), r.get("signal"), r.get("aux"), (_aux(i) + RUN_AUX) if isinstance(nm, str) else _aux(i))
    del got
    _opt(b"inflate_par", 2)
    try:
        alone = press.decode_records(streams, press.REC_ZLIB, press.SIG_EX_ZD, raise_on_error=False)
    finally:
        _opt(b"inflate_par", 1)
    assert [g_["status"] == 8 for g_ in alone] == [isinstance(nm, str) for nm in names]


@pytest.mark.gpu
@pytest.mark.parametrize("lds", [0, 1])
def test_no_payload_forms(press, batch, lds):
    """k_inflate_par_np with the ex-zd wave decoder, np_lds_payload 0 and 1: ex-zd has no LDS-payload kernel, so either setting
    inflates each record into its workgroup's scratch slot and decodes from there.  Three slots of scratch: two for the main
    kernel, one for k_inflate_fallback_np — that one stays untouched (no record declined), the two main ones hold payload bytes"""
    names, blobs, pays, streams = batch
    cap = _np_cap(pays)
    _opt(b"np_lds_payload", lds)
    try:
        f, sig, scr = _dev(streams, "np", _sig_caps(names, blobs), rec_method=1, np_cap=cap, max_in_len=max(map(len, streams)))
    finally:
        _opt(b"np_lds_payload", 1)
    _check_dev(names, f, sig)
    slot = (cap + 31) & ~15
    assert (scr[64 + 2 * slot:64 + 3 * slot] == 0xA5).all()
    assert (scr[64:64 + slot] != 0xA5).any() and (scr[64 + slot:64 + 2 * slot] != 0xA5).any()


@pytest.mark.gpu
def test_zstd_records(press, batch):
    """k_zstd_inflate<2> (the decoding wave runs exzd_decode_wave) and unpack_fused = 0 (k_unpack -> exzd_decode_wg behind
    k_zstd_inflate<0>)"""
    if ob.zstd_ref() is not None:
        compress = ob.zstd_compress
    elif hasattr(ob.lib(), "s5o_zstd_literals_compress"):
        compress = ob.zstd_literals_compress
    else:
        pytest.skip("neither libzstd.so.1 nor the oracle's zstd encoder in this image")
    names, blobs, pays, _ = batch
    frames = [compress(p) for p in pays]
    _check_host(names, press.decode_records(frames, press.REC_ZSTD, press.SIG_EX_ZD, raise_on_error=False), pays)
    f, sig, _ = _dev(frames, "full", _sig_caps(names, blobs), rec_method=2, pay_caps=[len(p) + 64 for p in pays])
    _check_dev(names, f, sig)
    _opt(b"unpack_fused", 0)
    try:
        _check_host(names, press.decode_records(frames, press.REC_ZSTD, press.SIG_EX_ZD, raise_on_error=False), pays)
    finally:
        _opt(b"unpack_fused", 1)


def _solo():
    from slow5tools_amd import _lib
    L = _lib.lib()
    L.slow5_ptr_depress_solo.restype = C.c_void_p
    L.slow5_ptr_depress_solo.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    return L, libc


@pytest.mark.gpu
def test_solo_depress_batch(press, batch):
    """s5gpu_solo_batch stage 7: the host sizes each slot from the blob's count (clamped by its bytes) and retries a status 6 with the
    count reported — an impossible count must end as 7, with no buffer"""
    L, libc = _solo()
    names, blobs = batch[:2]
    n = len(blobs)
    bufs = [C.create_string_buffer(b, max(len(b), 1)) for b in blobs]
    inp = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in blobs])
    out, olen, st = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int32 * n)()
    rc = L.s5gpu_solo_batch(7, n, inp, lens, out, olen, st)
    assert rc == -5    # S5GPU_ERR_DATA: some inputs are corrupt
    for i, nm in enumerate(names):
        s = np.frombuffer(C.string_at(out[i], olen[i]), dtype=np.int16) if out[i] else None
        if out[i]:
            libc.free(out[i])
        _check(nm, st[i], olen[i] // 2, s)
        if isinstance(nm, str) and nm in MALFORMED:
            assert s is None and olen[i] == 0, nm


@pytest.mark.gpu
def test_solo_depress_single_calls(press):
    """slow5_ptr_depress_solo(SLOW5_COMPRESS_EX_ZD): NULL for a malformed blob, the exact bytes otherwise"""
    L, libc = _solo()
    EX_ZD = 4
    for name, blob in CORPUS:
        cnt = C.c_size_t(12345)
        p = L.slow5_ptr_depress_solo(EX_ZD, blob, len(blob), C.byref(cnt))
        if REF[name] is None:
            assert not p, name
        else:
            assert p and cnt.value == 2 * len(REF[name]), name
            got = np.frombuffer(C.string_at(p, cnt.value), dtype=np.int16)
            libc.free(p)
            assert np.array_equal(got, REF[name]), name


@pytest.mark.gpu
def test_valid_blob_in_too_small_a_signal_slot(press):
    """a signal slot one sample short: status 6 with the blob's count and nothing written behind the slot (the sentinels of
    _dev_decode), from k_unpack (exzd_decode_wg), k_inflate_par<2> and k_inflate_par_np (exzd_decode_wave); with N samples it decodes"""
    pick = ["n1", "n2_exception", "last_tile_1", "last_tile_17", "nex4097", "chunk_cut_512", "all_exceptions_n600", "non_minimal_widths", "q15"]
    blobs = [dict(CORPUS)[n] for n in pick]
    g = _guards(len(pick) + 1)
    all_blobs = _interleave(blobs, g)
    wants = _interleave([REF[n] for n in pick], [ref_decode(x) for x in g])
    short = [len(w) - 1 if k % 2 else len(w) for k, w in enumerate(wants)]
    exact = [len(w) for w in wants]
    pays = [_payload(b, i) for i, b in enumerate(all_blobs)]
    streams = [zlib.compress(p, 6) for p in pays]
    pc = [len(p) + 64 for p in pays]
    cap = _np_cap(pays)
    for recs, form, kw in ((pays, "full", dict(rec_method=0, pay_caps=pc)), (streams, "full", dict(rec_method=1, pay_caps=pc)),
                           (streams, "np", dict(rec_method=1, np_cap=cap, max_in_len=max(map(len, streams))))):
        f, sig, _ = _dev(recs, form, short, **kw)
        for k, w in enumerate(wants):
            if k % 2:
                assert f["status"][k] == 6 and f["n_samples"][k] == len(w), (form, k, int(f["status"][k]))
            else:
                assert f["status"][k] == 0 and np.array_equal(sig[k], w), (form, k)
        f, sig, _ = _dev(recs, form, exact, **kw)
        assert all(f["status"] == 0) and all(np.array_equal(s, w) for s, w in zip(sig, wants)), form
