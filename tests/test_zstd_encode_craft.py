"""Every launch route of the zstd record ENCODER (csrc/zstd_enc_dev.h: zstd_tokenise, zstd_block, zstd_desc_*, zstd_sequences_wave,
zstd_record; k_zstd_fused<EXZD> and k_zstd_staged) on hand-made payloads, parsed block by block.

tests/zstd_craft.py holds the infrastructure: parse_frame reads a frame down to header fields, tree description, stream sizes and sequences;
zenc_pieces / zenc_tokens restate what the encoder MUST do (where it cuts, which runs are sequences, when it takes them); zenc_catalogue()
names the smallest payloads that reach each of its edges.  The CPU tests pin the parser on the decoders' catalogue, on libzstd's frames and on
the CPU twin's, the restatement on the payloads, and every entry's stated property on the restatement alone.  The GPU tests send the
catalogue, every entry at four consecutive positions (role = (wave + blockIdx.x) & 3 takes all four values), through

  route          call                                                         kernels
  solo           s5gpu_solo_batch(5, ...)                                     k_zstd_staged over whole buffers
  fused          encode(), REC_ZSTD, svb-zd, budget 16384                     k_zstd_fused<false>
  exzd           the same with SIG_EX_ZD                                      k_zstd_fused<true>
  overflow       encode() with a budget below every payload                   fused declines all, then k_pack + k_zstd_staged over the list
  all-staged     encode() of a batch with one long read, no budget named      k_pack + k_zstd_staged
  parked         pack_parked() + deflate_parked()                             k_zstd_staged
  host           press.encode_records                                         what s5gpu_encode_batch plans
  literals-only  fused and overflow with option zstd_sequences = 0            the split form of zstd_record<false>; blocks without sequences

and hold every record of every route to what _check_frame and _check_block say.
"""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import deflate_craft as dc
import oracle_bind as ob
import zstd_craft as zc
from test_oracle_golden import zstd_test_inputs

SMALL_INPUTS = (10, 100, 1000, 5000, 40000)          # sizes of zstd_test_inputs used here (the parser is plain Python)


def _payload(e, sm=1):
    return zc.zenc_payload(e, sm)


# ---------------------------------------------------------------- CPU: the parser
MODE_BITS = {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}


def test_parse_frame_on_the_decoder_catalogue():
    """every valid frame of CATALOGUE parses to its content with nothing trailing (but the one made of two frames), block by block what the
    builder was given: block types, literals kinds and bytes, sequence counts and triples, the modes byte; every frame that must be refused
    raises, but for the rows tagged STRICTER (what libzstd 1.4.8 lets pass; parse_frame may go either way)"""
    n = 0
    for name, data, expected, tags in zc.CATALOGUE:
        if expected is None:
            if zc.STRICTER not in tags:
                with pytest.raises(ValueError):
                    zc.parse_frame(data)
            continue
        f = zc.parse_frame(data)
        assert f.content == expected and f.trailing == b"", name
        spec = zc.SPECS[data]
        assert len(f.blocks) == len(spec) and [b.last for b in f.blocks] == [False] * (len(spec) - 1) + [True], name
        for b, s in zip(f.blocks, spec):
            assert b.type == {"raw": 0, "rle": 1, "comp": 2}[s["kind"]], name
            if s["kind"] == "comp":
                assert b.lit.kind == s["lits"]["kind"] and b.literals == s["lits"]["data"] and b.lit.regen == len(b.literals), name
                assert b.nseq == len(s["seqs"]) and b.seqs == [tuple(x) for x in s["seqs"]], name
                if s["lits"]["kind"] in ("huf", "treeless"):
                    assert b.lit.streams == s["lits"]["streams"] and b.lit.desc_exact, name
                    if s["lits"]["kind"] == "huf":
                        assert b.lit.desc == s["lits"]["desc"], name
                if b.nseq:
                    want = 0
                    for m, shift in zip(s["modes"], (6, 4, 2)):
                        want |= MODE_BITS[m if isinstance(m, str) else m[0]] << shift
                    assert b.modes == want and b.nseq_bytes == s["forge"].get("nseq_bytes", 1 if b.nseq < 128 else 2 if b.nseq < 0x7F00 else 3), name
        n += 1
    assert n > 64
    two = next(d for nm, d, _, _ in zc.CATALOGUE if nm == "two frames back to back")
    assert zc.parse_frame(two).trailing == two[len(two) // 2:]


def test_parse_frame_on_libzstd_frames():
    """frames of libzstd at levels 1, 3, 9, 19 and -5: the input back, nothing trailing, every FSE stream of weights ending exactly"""
    if ob.zstd_ref() is None:
        pytest.skip("no libzstd.so.1 in this image")
    kinds = set()
    for d in zstd_test_inputs(np.random.default_rng(21), sizes=SMALL_INPUTS):
        for level in (1, 3, 9, 19, -5):
            f = zc.parse_frame(ob.zstd_compress(d, level))
            assert f.content == d and f.trailing == b"" and (f.fcs is None or f.fcs == len(d)), (len(d), level)
            assert all(b.lit is None or b.lit.desc_exact for b in f.blocks), (len(d), level)
            kinds |= {(b.type, b.lit.kind if b.lit else None) for b in f.blocks}
    assert kinds >= {(0, None), (2, "raw"), (2, "huf")}, kinds


def test_parse_frame_on_the_cpu_twin():
    """frames of oracle/zstd_enc.c (the device encoder's layout, stated on the CPU): the input back"""
    for d in zstd_test_inputs(np.random.default_rng(22), sizes=SMALL_INPUTS):
        fr = ob.zstd_literals_compress(d)
        f = zc.parse_frame(fr)
        assert f.content == d and f.trailing == b"" and f.fcs == len(d), len(d)


def test_package_merge_is_optimal_where_huffman_fits():
    """limited_lengths against the plain Huffman construction (same cost wherever that stays within the limit), a complete code always, and the
    limit kept on a Fibonacci-like histogram that plain Huffman would give 20 bits"""
    rng = np.random.default_rng(5)
    for k in (2, 3, 17, 100, 256):
        h = [0] * 256
        for s in rng.choice(256, k, replace=False):
            h[s] = int(rng.integers(1, 500))
        plain = dc.huff_lengths(h, 32)
        lim = zc.limited_lengths(h, 15)
        assert zc.kraft(lim, 15) == 1 << 15 and max(lim) <= 15
        if max(plain) <= 15:
            assert zc.code_bits(h, lim) == zc.code_bits(h, plain), k
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946]
    lim = zc.limited_lengths(fib, 11)
    assert max(lim) == 11 and zc.kraft(lim) == 1 << 11 and max(dc.huff_lengths(fib, 32)) == 20


# ---------------------------------------------------------------- CPU: the restatement and the catalogue
def _expand(lits, seqs):
    out, li = bytearray(), 0
    for ll, ml in seqs:
        out += lits[li:li + ll]
        li += ll
        out += out[-1:] * ml
    return bytes(out + lits[li:])


def test_restated_tokens_expand_to_every_payload():
    """the restated literals and sequences of every block of every entry (svb-zd and ex-zd payload) are that block; every literal length is
    at least 1 and every match at least 4; the pieces are the payload"""
    for e in zc.zenc_catalogue():
        if len(_payload(e)) > 1 << 20:
            continue
        for sm in (1,) if e["solo"] else (1, 2):
            p = _payload(e, sm)
            assert b"".join(zc.zenc_pieces(p)) == p and all(len(x) == zc.ZBLOCK for x in zc.zenc_pieces(p)[:-1]) and 0 < len(zc.zenc_pieces(p)[-1]) <= zc.ZBLOCK or not p, e["name"]
            for piece in zc.zenc_pieces(p):
                lits, seqs, taken = zc.zenc_tokens(piece)
                assert _expand(lits, seqs) == piece and all(ll >= 1 and ml >= 4 for ll, ml in seqs), (e["name"], sm)
                assert not taken or len(piece) >= 64
    assert zc.zenc_pieces(b"") == [b""] and zc.zenc_tokens(b"") == (b"", [], False)
    assert zc.zenc_tokens(b"abbbbbc" * 20)[:2] == (b"abc" * 20, [(2, 4)] + [(3, 4)] * 19)


def test_the_crafted_set_covers_every_edge_it_names():
    """asserted on the CPU, from the payloads and the restatement alone, before any GPU test relies on it: every entry's stated property holds,
    every edge an entry claims is one of ZENC_EDGES, and every edge of ZENC_EDGES is claimed"""
    cat = zc.zenc_catalogue()
    assert len({e["name"] for e in cat}) == len(cat) and all(e["why"] and e["edges"] for e in cat)
    claimed = set()
    for e in cat:
        assert e["prop"](zc.ZView(_payload(e))) is True, e["name"]
        assert set(e["edges"]) <= set(zc.ZENC_EDGES), e["name"]
        claimed |= set(e["edges"])
        assert len(_payload(e)) <= 33000 or e["name"] == "size_16777221", e["name"]
    assert claimed == set(zc.ZENC_EDGES), sorted(set(zc.ZENC_EDGES) - claimed)
    assert len(zc.ZENC_EDGES) == len(set(zc.ZENC_EDGES))
    # the three lane chunks are the smallest, a middle one and the largest; every record entry can ride the fused kernel or is a multi-block one
    assert [zc.zenc_chunk(n) for n in (64, 1024, 1025, 15360, 15361, 16384)] == [4, 4, 8, 60, 64, 64]
    assert sum(1 for e in cat if not e["solo"]) >= 50 and sum(1 for e in cat if not e["solo"] and len(_payload(e)) > zc.ZBLOCK) >= 5


def _families():
    fam = {}
    for e in zc.zenc_catalogue():
        fam.setdefault(zc.zenc_family(e["name"]), []).append(e)
    return fam


def test_docs_list_every_family_of_encoder_entries():
    """docs/codecs.md has one table row per family of entries (the names of one loop of the catalogue, numbers written #):
    | zstd | `family` | entries | payload bytes lo .. hi | what its first entry reaches |"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "docs", "codecs.md"), encoding="utf-8").read()
    rows = {m.group(1): m.groups()[1:] for m in re.finditer(r"^\| zstd \| `([\w#]+)` \| (\d+) \| (\d+) \.\. (\d+) B \| (.*) \|$", text, re.M)}
    fam = _families()
    for name, ents in fam.items():
        sizes = [len(_payload(e)) for e in ents]
        assert rows.get(name) == (str(len(ents)), str(min(sizes)), str(max(sizes)), ents[0]["why"]), name
    assert len(rows) == len(fam) < 80
    assert "%d entries" % len(zc.zenc_catalogue()) in text and "%d named edges" % len(zc.ZENC_EDGES) in text


# ---------------------------------------------------------------- what every record is held to
_CHECKED = {}                     # (frame, payload, mode) -> what its blocks showed: a frame equal to one already parsed needs only the identity


def _bits_bound(lits):
    """Upper bound of the bits the encoder's code may spend on these literals.  Its lengths come from assign_lengths_wave<11>, which starts at
    min(11, ceil(log2(N / f))) and only ever shortens the code of a symbol in use: wherever those clamped Shannon lengths are a code (Kraft sum
    <= 1) the bits are at most sum f * min(11, ceil(log2(N / f))) — and the exact construction, taken for up to 16 symbols, is a Huffman code,
    which no code undercuts, so the bound holds for it too as long as its tree stays within 11 bits.  Where the clamped lengths over-subscribe
    the code space, build_lengths makes a Huffman tree, cuts it at 11 bits and repairs the Kraft sum by lengthening other codes: the yardstick
    is the test's own optimal 11-bit-limited code (package-merge) with no factor on it, plus 11 bits for every literal whose Shannon length
    exceeds 11 — the clamp touches only those symbols, and the room the repair makes for them is at most what their own 11-bit codes take."""
    h = zc.histogram(lits)
    sl = zc.shannon_clamped(h)
    if zc.kraft(sl) <= 1 << zc.ZMAXBITS and (sum(1 for f in h if f) > 16 or max(dc.huff_lengths(h, 64)) <= zc.ZMAXBITS):
        return zc.code_bits(h, sl)
    N = sum(h)
    return zc.code_bits(h, zc.limited_lengths(h)) + 11 * sum(f for f in h if f and (f << zc.ZMAXBITS) < N)


def _check_huffman(b, lits, where):
    L, nl = b.lit, len(lits)
    assert L.streams == 4 and L.sf in (1, 2, 3) and nl >= 64, where
    h = zc.histogram(lits)
    top = max(s for s, f in enumerate(h) if f)
    assert len(L.lengths) == top + 1 and max(L.lengths) <= zc.ZMAXBITS and all(L.lengths[s] for s, f in enumerate(h) if f), where
    assert zc.kraft(L.lengths) == 1 << zc.ZMAXBITS, where                                        # the weights complete to a power of two: a complete code
    assert (L.desc == "direct") == (top <= 128) and L.desc_exact, (where, L.desc, top)
    per = (nl + 3) // 4
    shares = [lits[k * per:(k + 1) * per] for k in range(3)] + [lits[3 * per:]]
    bits = [sum(L.lengths[x] for x in s) for s in shares]
    assert list(L.stream_sizes) == [(x + 1 + 7) // 8 for x in bits], (where, L.stream_sizes, bits)
    assert L.csize == L.desc_len + 6 + sum(L.stream_sizes), where
    assert L.hl == (3 if nl <= 1023 and L.csize <= 1023 else 4 if nl <= 16383 and L.csize <= 16383 else 5), (where, nl, L.csize, L.hl)
    bound = _bits_bound(lits)
    assert sum(bits) <= bound, (where, sum(bits), bound)
    w = L.weights
    return {"norm_gives" if zc.normalise_sum(w) < 64 else "norm_takes" if zc.normalise_sum(w) > 64 else "norm_exact"} | {"gap_%d" % g for g in zc.weight_gaps(w)} \
        if L.desc == "fse" else {"direct_odd" if (len(w) - 1) & 1 else "direct_even"}


def _check_block(b, piece, where, seq_on=True, force_raw=False):
    """-> the classes the block belongs to"""
    blen = len(piece)
    lits, seqs, taken = zc.zenc_tokens(piece) if seq_on and not force_raw else (piece, [], False)
    if not taken:
        lits, seqs = piece, []
    nl, one = len(lits), len(set(piece)) == 1
    assert b.data == piece, where
    if force_raw:
        assert b.type == 0 and b.size == blen, where
        return {"raw_head"}
    assert (b.type == 1) == (blen >= 64 and one and not taken), (where, b.type)                   # an RLE block for a single-byte block of >= 64 bytes, only
    if b.type == 1:
        return {"rle_block"}
    assert taken <= (b.type == 2), (where, "sequences refused that the rule takes")
    if b.type == 0:
        assert b.size == blen, where
        # raw although the encoder's own Huffman section was certainly small enough?
        assert not zc.huffman_certain(piece, blen), (where, "a raw block where hl + csize + 1 < blen was certain")
        return {"raw_block"}
    assert b.size < blen, (where, b.size, blen)
    assert b.literals == lits and b.lit.regen == nl, where
    cls = {"compressed"}
    if taken:
        assert b.nseq == len(seqs) and [(ll, ml) for ll, ml, _ in b.seqs] == seqs, (where, b.nseq, len(seqs))
        assert all(ofv == 1 and ll >= 1 for ll, _, ofv in b.seqs), where
        assert b.modes == 0x10 and b.rle_codes == {"of": 0} and b.nseq_bytes == (1 if b.nseq < 128 else 2), (where, b.modes, b.rle_codes)
        cls |= {"sequences", "count_%d" % b.nseq_bytes}
    else:
        assert b.nseq == 0 and b.nseq_bytes == 1 and b.lit.kind == "huf", where                   # without sequences only Huffman literals make a compressed block
    rawl = (1 if nl < 32 else 2 if nl < 4096 else 3) + nl
    assert b.lit.kind in ("raw", "huf"), (where, b.lit.kind)                                      # (RLE literals beside sequences: unreachable, see zenc_catalogue)
    if b.lit.kind == "raw":
        assert b.lit.hl == rawl - nl, where
        assert not (nl >= 64 and len(set(lits)) > 1 and zc.kraft(zc.shannon_clamped(zc.histogram(lits))) <= 1 << zc.ZMAXBITS and zc.huffman_ceiling(lits) < rawl), \
            (where, "raw literals where hl + csize < rawl was certain")
        cls.add("lit_raw_%d" % b.lit.hl)
    else:
        cls |= _check_huffman(b, lits, where)
        if taken:
            assert b.lit.hl + b.lit.csize < rawl, (where, b.lit.hl, b.lit.csize, rawl)
        else:
            assert b.lit.hl + b.lit.csize + 1 < blen, (where, b.lit.hl, b.lit.csize, blen)
        cls.add("lit_huf_%d" % b.lit.hl)
    return cls


def _check_frame(where, frame, payload, want=None, seq_on=True, raw_head=False, only=None):
    """want: the blocks' bytes (default: one per 16384 bytes); only: indices of the blocks to check (the 16 MiB frame)"""
    key = (frame, payload, seq_on, raw_head)
    if key in _CHECKED:
        return _CHECKED[key]
    assert frame[:4] == zc.MAGIC and frame[4] == 0xA0 and struct.unpack_from("<I", frame, 5)[0] == len(payload), where
    F = zc.parse_frame(frame)
    assert F.trailing == b"" and F.fcs == len(payload) and F.fcs_bytes == 4 and F.checksum is None, where
    assert F.content == payload, where
    assert ob.zstd_restated_decompress(frame, len(payload)) == payload, where
    if ob.zstd_ref() is not None:
        assert ob.zstd_decompress(frame, len(payload)) == payload, where
    want = zc.zenc_pieces(payload) if want is None else want
    assert [len(b.data) for b in F.blocks] == [len(x) for x in want], (where, [len(b.data) for b in F.blocks][:8])
    assert [b.last for b in F.blocks] == [False] * (len(want) - 1) + [True], where
    cls, starts, at = set(), [], 9
    for k, (b, piece) in enumerate(zip(F.blocks, want)):
        starts.append(at)
        at += 3 + (1 if b.type == 1 else b.size)
        if only is None or k in only:
            cls |= _check_block(b, piece, where + (k,), seq_on, raw_head and k == 0)
    assert at == len(frame), where
    _CHECKED[key] = (cls, starts)
    return _CHECKED[key]


def _record_frame(where, rec):
    (sz,) = struct.unpack_from("<Q", rec, 0)
    assert sz == len(rec) - 8, where
    return rec[8:]


# ---------------------------------------------------------------- the device
COPIES = 4                        # consecutive positions of every entry in every batch: blockIdx.x & 3 takes every value


@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


def _solo(stage, items):
    """s5gpu_solo_batch: whole buffers in, (rc, buffers or None, status) out — stage 5 compresses to zstd frames, 4 reads them"""
    from slow5tools_amd import _lib
    L = _lib.lib()
    n = len(items)
    bufs = [C.create_string_buffer(d, len(d)) if len(d) else C.create_string_buffer(1) for d in items]
    inp = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * n)(*[len(d) for d in items])
    out, olen, st = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int32 * n)()
    rc = L.s5gpu_solo_batch(stage, n, inp, lens, out, olen, st)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    res = []
    for i in range(n):
        res.append(C.string_at(out[i], olen[i]) if out[i] else None)
        if out[i]:
            libc.free(out[i])
    return rc, res, list(st)


def _set_zseq(v):
    from slow5tools_amd import _lib
    _lib.check(_lib.lib().s5gpu_set_option(b"zstd_sequences", v), "zstd_sequences")


def _recs(sm=1, at_most=None):
    """the record entries (whose payload for signal method sm is at most at_most bytes)"""
    return [e for e in zc.zenc_catalogue() if not e["solo"] and (at_most is None or len(_payload(e, sm)) <= at_most)]


def _times(ents):
    return [e for e in ents for _ in range(COPIES)]


LONG_READ = 70000                 # samples of the read that makes a batch "long" (s5plan::all_staged: its payload bound exceeds four blocks by far)


def _device_batch(press, ents, cap, sm=1, long_read=False):
    """the entries as a DeviceBatch of zstd records; the slots filled with STALE_FILL (what lies behind a parked payload is then known)"""
    sigs = [np.asarray(e["signal"], dtype=np.int16) for e in ents]
    hdrs = [dc.enc_hdr(e) for e in ents]
    auxs = [e["aux"] for e in ents]
    if long_read:
        sigs.append(ob.synth_read(0x5105, 0, LONG_READ))
        hdrs.append(press.pack_hdr(b"long", 0, 8192.0, 23.0, 1467.61, 4000.0))
        auxs.append(b"")
    b = press.DeviceBatch([len(s) for s in sigs], hdr_len=[len(h) for h in hdrs], aux_len=[len(a) for a in auxs], rec_method=press.REC_ZSTD, sig_method=sm,
                          lds_payload_cap=cap, with_stream_out=False)
    b.upload(sigs, hdrs, auxs)
    fill = b.torch.tensor(list(zc.STALE_FILL[:4]), dtype=b.torch.uint8, device=b.dev)
    b.slots[:b.slots.numel() // 4 * 4].view(-1, 4)[:] = fill
    return b


_ROUTES = {}


def _route(press, name):
    """the records of a route, made once: [(entry, record)] with every entry COPIES times"""
    if name in _ROUTES:
        return _ROUTES[name]
    if name == "solo":
        ents = _times([e for e in zc.zenc_catalogue() if len(_payload(e)) < 1 << 20])
        rc, frames, st = _solo(5, [_payload(e) for e in ents])
        assert rc == 0 and not any(st)
        out = [(e, struct.pack("<Q", len(f)) + f) for e, f in zip(ents, frames)]
    elif name in ("fused", "exzd", "fused-literals-only"):
        sm = 2 if name == "exzd" else 1
        ents = _times(_recs(sm, zc.ZBLOCK))
        assert len(ents) >= 40 * COPIES
        b = _device_batch(press, ents, zc.ZBLOCK, sm)
        b.encode()
        out = list(zip(ents, b.records()))
        assert int(b.ovf[0].item()) == 0
    elif name in ("overflow", "overflow-literals-only"):
        ents = _times(_recs())
        b = _device_batch(press, ents, 48)
        b.encode()
        out = list(zip(ents, b.records()))
        assert int(b.ovf[0].item()) == len(ents)
    elif name == "all-staged":
        ents = _times(_recs())
        b = _device_batch(press, ents, 0, long_read=True)
        assert b.tot["max_payload"] * 100 // 325 > 4 * zc.ZBLOCK                                  # s5plan::all_staged holds
        b.encode()
        recs = b.records()
        raw = press.encode_records([ob.synth_read(0x5105, 0, LONG_READ)], [press.pack_hdr(b"long", 0, 8192.0, 23.0, 1467.61, 4000.0)], None, press.REC_NONE, press.SIG_SVB_ZD)
        assert ob.zstd_restated_decompress(_record_frame(("all-staged", "long"), recs[-1]), len(raw[0])) == raw[0][8:]
        out = list(zip(ents, recs[:-1]))
    elif name == "parked":
        ents = _times(_recs())
        b = _device_batch(press, ents, 0)
        b.pack_parked()
        b.deflate_parked()
        out = list(zip(ents, b.records()))
    else:
        assert name == "host"
        ents = _times(_recs())
        out = list(zip(ents, press.encode_records([np.asarray(e["signal"], dtype=np.int16) for e in ents], [dc.enc_hdr(e) for e in ents], [e["aux"] for e in ents],
                                                  press.REC_ZSTD, press.SIG_SVB_ZD)))
    _ROUTES[name] = out
    return out


# what the catalogue must have produced on a route that takes all of it: every block kind, both count widths, the raw literals headers, the Huffman
# headers, both description forms and both parities of the direct one, the zero-run flags of the count header, normalisation both ways
CLASSES_ALL = {"rle_block", "raw_block", "compressed", "sequences", "count_1", "count_2", "lit_raw_1", "lit_raw_2", "lit_raw_3", "lit_huf_3", "lit_huf_4", "lit_huf_5",
               "direct_odd", "direct_even", "gap_1", "gap_3", "gap_4", "gap_6", "norm_gives", "norm_takes"}
CLASSES_RECORDS = {"compressed", "sequences", "count_1", "count_2", "lit_huf_3", "lit_huf_4"}       # (a record's head holds bytes up to E0: FSE descriptions only)


def _check_route(name, recs, sm=1, need=CLASSES_RECORDS, **how):
    cls, n = set(), 0
    for k, (e, rec) in enumerate(recs):
        c, _ = _check_frame((name, e["name"], k % COPIES), _record_frame((name, e["name"]), rec), _payload(e, sm), **how)
        cls |= c
        n += 1
    print("%s: %d records, %d distinct frames so far, classes missing %s" % (name, n, len(_CHECKED), sorted(need - cls)))
    assert cls >= need, sorted(need - cls)
    return cls


@pytest.mark.gpu
def test_route_solo(press):
    """s5gpu_solo_batch(5): every entry but the 16 MiB one, the record payloads too, as whole buffers; the device decoder reads the frames back"""
    recs = _route(press, "solo")
    _check_route("solo", recs, need=CLASSES_ALL)
    frames = [r[8:] for _, r in recs[::COPIES]]
    rc, back, st = _solo(4, frames)
    assert rc == 0 and back == [_payload(e) for e, _ in recs[::COPIES]]


@pytest.mark.gpu
def test_route_solo_16_mib(press):
    """2^24 + 5 bytes once: the header (content size 05 00 00 01: the carry byte of the 4-byte field), the first and the last block, the content"""
    e = next(e for e in zc.zenc_catalogue() if e["name"] == "size_16777221")
    p = _payload(e)
    rc, (frame,), st = _solo(5, [p])
    assert rc == 0 and st == [0] and frame[4:9] == b"\xa0\x05\x00\x00\x01"
    cls, _ = _check_frame(("solo", e["name"]), frame, p, only=(0, 1024))
    assert cls >= {"compressed", "sequences", "raw_block"}, cls                                 # block 0 holds two literals in zeros; the last is five bytes
    F = zc.parse_frame(frame)
    assert sum(b.type == 1 for b in F.blocks) == 1024 - 2 and len(frame) < 5000


@pytest.mark.gpu
def test_route_fused(press):
    """encode() with a budget of one block: every record entry of at most 16384 bytes in k_zstd_fused<false>, nothing on the overflow list"""
    _check_route("fused", _route(press, "fused"))


@pytest.mark.gpu
def test_route_exzd(press):
    """the same with SIG_EX_ZD: k_zstd_fused<true> builds another blob in front of the same aux bytes; the payload is the oracle's rec_pack(r, 2)"""
    _check_route("exzd", _route(press, "exzd"), sm=2)


@pytest.mark.gpu
def test_route_overflow_list(press):
    """encode() with a budget below the shortest payload: the fused launch declines every read, k_zstd_staged takes them from the list"""
    _check_route("overflow", _route(press, "overflow"))


@pytest.mark.gpu
def test_route_all_staged(press):
    """a batch with one long read and no budget named: s5plan::all_staged, k_pack + k_zstd_staged over every read"""
    _check_route("all-staged", _route(press, "all-staged"))


@pytest.mark.gpu
def test_route_parked(press):
    """pack_parked() + deflate_parked()"""
    _check_route("parked", _route(press, "parked"))


@pytest.mark.gpu
def test_route_host(press):
    """press.encode_records: what s5gpu_encode_batch makes of the record entries in one call; the device decoder reads the records back"""
    recs = _route(press, "host")
    _check_route("host", recs)
    one = recs[::COPIES]
    dec = press.decode_records([r[8:] for _, r in one], press.REC_ZSTD, press.SIG_SVB_ZD)
    for (e, _), d in zip(one, dec):
        assert d["status"] == 0 and np.array_equal(d["signal"], np.asarray(e["signal"], dtype=np.int16)) and d["aux"] == e["aux"], e["name"]


@pytest.mark.gpu
def test_route_literals_only(press):
    """option zstd_sequences = 0: no block holds a sequence.  Fused, svb-zd: a record whose key bytes end at `at` with at >= 256 and
    at + 256 <= plen goes out as a raw head block of hdr_len + 12 bytes, a key block up to `at` and the rest (zenc_split) — the blocks start
    at every alignment in LDS; staged: whole blocks as ever"""
    try:
        _set_zseq(0)
        fused = _route(press, "fused-literals-only")
        staged = _route(press, "overflow-literals-only")
    finally:
        _set_zseq(1)
    splits = set()
    for k, (e, rec) in enumerate(fused):
        p = _payload(e)
        cut = zc.zenc_split(e["hdr_len"], len(e["signal"]), len(p))
        want = None
        if cut is not None:
            ends = np.cumsum(cut).tolist()
            want = [p[a:b] for a, b in zip([0] + ends, ends)]
            splits.add(cut[0] % 4)
        _check_frame(("fused-literals-only", e["name"], k % COPIES), _record_frame((e["name"],), rec), p, want=want, seq_on=False, raw_head=cut is not None)
    assert splits == {0, 1, 2, 3}
    _check_route("overflow-literals-only", staged, seq_on=False, need={"compressed", "lit_huf_3", "lit_huf_4"})


@pytest.mark.gpu
def test_every_route_writes_the_same_frame(press):
    """nothing in the kernels makes the output depend on the route, on the workgroup's index or on which wave played which role: the four
    copies of an entry are one frame; solo, overflow, all-staged, parked and host records of a payload are one frame, and so is the fused
    record of a payload of at most a block"""
    by = {}
    for name in ("solo", "fused", "overflow", "all-staged", "parked", "host"):
        recs = _route(press, name)
        for k in range(0, len(recs), COPIES):
            e = recs[k][0]
            assert len({r for _, r in recs[k:k + COPIES]}) == 1, (name, e["name"], "the copies differ")
            by.setdefault(e["name"], {})[name] = recs[k][1]
    n = 0
    for ename, got in by.items():
        assert len(set(got.values())) == 1, (ename, {k: len(v) for k, v in got.items()})
        n += len(got) > 1
    assert n >= 50


@pytest.mark.gpu
def test_second_block_starts_at_every_byte_phase(press):
    """the four align_phase entries: their second block's header starts at all four byte phases of a word of the record slot"""
    recs = dict((e["name"], r) for e, r in _route(press, "parked"))
    phases = set()
    for k in range(4):
        e = next(e for e in zc.zenc_catalogue() if e["name"] == "align_phase_%d" % k)
        _, starts = _check_frame(("parked", e["name"], 0), recs[e["name"]][8:], _payload(e))
        phases.add((8 + starts[1]) % 4)
    assert phases == {0, 1, 2, 3}
