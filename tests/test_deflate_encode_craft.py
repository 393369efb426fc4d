"""Every launch route of the zlib record ENCODER (deflate_block2, csrc/deflate2_dev.h) on hand-made payloads, parsed token by token.

A record's aux bytes are copied verbatim behind the signal blob, so the payload behind the head is the test's to choose:
tests/deflate_craft.py's encode_catalogue() names the smallest payloads that reach each edge of the encoder (slab, lane, wave-region and
block boundaries, the token list's 640 entries and its second pool, the code-length header's chunks, the block choice).  The CPU tests
pin the parser on stock zlib, the restated tokeniser on the payloads, and every entry's stated property on the restatement alone.  The
GPU tests send the catalogue through

  route      call                                                         kernels
  fused      encode(), budget 8192 | 16384                                k_encode_fused<uint32_t> | <uint64_t>: deflate_block2<1>
  stream     encode_stream(), the same two batches                        k_encode_stream<uint32_t> | <uint64_t>
  parked     pack_parked() + deflate_parked(), every entry                k_pack + k_deflate_staged: deflate_block2<2, 256>
  overflow   encode() with a budget below every payload                   k_encode_fused (declines all) + k_pack + k_deflate_staged over the list
  tier2      encode(), budget 2048, option fused_tier2 = 16384            two fused launches (the second k_encode_fused<uint64_t, false, 4>), the rest staged
  host       press.encode_records                                         what s5gpu_encode_batch plans
  exzd       encode() and encode_stream() with SIG_EX_ZD, budget 8192     k_encode_fused<uint32_t, true>, k_encode_stream<uint32_t, true>

and hold every record of every route to: the size prefix; stock zlib inflates it to the oracle's payload with nothing behind the Adler-32;
one block per 16384 bytes of payload, its tokens exactly the restated ones; the block choice inequalities; for dynamic blocks the
lit/len code (<= 15 bits, complete, a code for every symbol in use, body no larger than at its Shannon start), the two 1-bit distance
codes, HLIT, the code-length entries as cl_rle gives them and the cheaper of the two static code-length codes.
"""
import contextlib
import os
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as dc

ZV = "zlib " + zlib.ZLIB_RUNTIME_VERSION
NARROW = 8192                                  # s5plan::NARROW_MAX: fused budgets up to here run the uint32_t kernels


def _payload(e, sm=1):
    return dc.enc_payload(e, sm)


# ---------------------------------------------------------------- CPU: the parser
def _data(rng, n):
    return bytes(np.repeat(rng.integers(0, 40, n, dtype=np.uint8), rng.integers(1, 9, n)))


def test_parse_blocks_reproduces_stock_zlib_streams():
    """streams of stock zlib at levels 1, 6 and 9 (and level 0: stored blocks): parse_blocks gets the bytes, emit_blocks writes the very
    stream again from what it returned, and its tokens, written as fixed blocks by Stream(), inflate in stock zlib to the same bytes"""
    rng = np.random.default_rng(23)
    for data in (b"", b"a", _data(rng, 50), _data(rng, 7000), bytes(rng.integers(0, 256, 3000, dtype=np.uint8)), bytes(70000)):
        for level in (0, 1, 6, 9):
            s = zlib.compress(data, level)
            p = dc.parse_blocks(s)
            assert p.data == data and p.adler == zlib.adler32(data) and p.trailing == b"", (len(data), level, ZV)
            assert dc.emit_blocks(p) == s, (len(data), level, ZV)
            assert p.blocks[-1].bfinal and p.blocks[0].first_bit == 0 and all(a.end_bit == b.first_bit for a, b in zip(p.blocks, p.blocks[1:]))
            st = dc.Stream()
            for b in p.blocks:
                if b.btype == 0:
                    st.stored(b.data, final=b.bfinal)
                else:
                    st.fixed(dc.as_stream_tokens(b.tokens), final=b.bfinal)
            assert st.valid and dc.referee(st.zlib()) == data, (len(data), level, ZV)


NOT_AN_ENCODERS_CHOICE = {"len_258_as_284_plus_31", "len_sym_284"}       # length 258 written as symbol 284 + extra 31


def test_parse_blocks_reproduces_stream_built_streams():
    """the valid streams of the decoders' catalogue (Stream(): stored, fixed and dynamic blocks at any bit offset, code-length
    sequences in every mode, incomplete one-code sets): the bytes, and the stream again bit for bit — but for the two entries that write
    a length as no encoder does; a stream with bytes behind the Adler-32 reports them"""
    n = 0
    for e in dc.catalogue():
        if e.expected is None:
            continue
        p = dc.parse_blocks(e.stream)
        assert p.data == e.expected and p.trailing == b"", e.name
        assert [b.btype for b in p.blocks] == dc.py_inflate(e.stream).blocks, e.name
        assert (dc.emit_blocks(p) == e.stream) == (e.name not in NOT_AN_ENCODERS_CHOICE), e.name
        n += 1
    assert n > 150
    tail = dc.by_name()["bytes_behind_the_adler"]
    assert dc.parse_blocks(tail.stream).trailing == tail.stream[-3:]
    for name in ("block_type_3", "hlit_287", "code_length_code_incomplete", "too_far_first_token", "cut_in_literal", "header_cm_7"):
        with pytest.raises(ValueError):
            dc.parse_blocks(dc.by_name()[name].stream)


def test_cl_rle_on_the_cases_of_rfc_1951():
    """RFC 1951 3.2.7: "codes 8, 16 (+2 bits 11), 16 (+2 bits 10) will expand to 12 code lengths of 8 (1 + 6 + 5)"; 16 copies 3 - 6
    times, 17 repeats a zero 3 - 10 times, 18 repeats it 11 - 138 times; and the chunks of the rule written out by hand"""
    assert dc.cl_rle([8] * 12) == [(8, 0), (16, 3), (16, 2)]
    assert dc.cl_rle([5]) == [(5, 0)] and dc.cl_rle([5] * 3) == [(5, 0)] * 3 and dc.cl_rle([5] * 4) == [(5, 0), (16, 0)]
    assert dc.cl_rle([5] * 7) == [(5, 0), (16, 3)] and dc.cl_rle([5] * 8) == [(5, 0), (16, 3), (5, 0)]
    assert dc.cl_rle([5] * 10) == [(5, 0), (16, 3), (16, 0)] and dc.cl_rle([5] * 9) == [(5, 0), (16, 3), (5, 0), (5, 0)]
    assert dc.cl_rle([0, 0]) == [(0, 0)] * 2 and dc.cl_rle([0] * 3) == [(17, 0)] and dc.cl_rle([0] * 10) == [(17, 7)]
    assert dc.cl_rle([0] * 11) == [(18, 0)] and dc.cl_rle([0] * 138) == [(18, 127)]
    assert dc.cl_rle([0] * 139) == [(18, 127), (0, 0)] and dc.cl_rle([0] * 140) == [(18, 127), (0, 0), (0, 0)]
    assert dc.cl_rle([0] * 141) == [(18, 127), (17, 0)] and dc.cl_rle([0] * 149) == [(18, 127), (18, 0)]
    assert dc.cl_rle([3, 0, 0, 0, 3, 3, 0, 7, 7, 7, 7, 1, 1]) == [(3, 0), (17, 0), (3, 0), (3, 0), (0, 0), (7, 0), (16, 0), (1, 0), (1, 0)]
    for lens in ([8] * 12, [0] * 141 + [4] * 9 + [0, 0, 9], dc.FLAT286 + [1, 1], dc.ONE_PREFIX + dc.DIST30):         # and it says what it stands for
        back = []
        for s, x in dc.cl_rle(lens):
            back += [s] if s < 16 else [back[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
        assert back == lens
    assert sum(1 << (7 - l) for l in dc.CLA_LENS if l) == 128 and sum(1 << (7 - l) for l in dc.CLB_LENS) == 128      # both complete


# ---------------------------------------------------------------- CPU: the catalogue
def test_rle_tokens_expand_to_every_payload():
    """the restated tokens of every block of every entry (svb-zd and ex-zd payload) are that block, token for token: a literal is the
    byte, a match has distance 1 and 3 .. 258 bytes, and no two tokens could have been one"""
    for e in dc.encode_catalogue():
        for sm in (1, 2):
            for piece in dc.pieces(_payload(e, sm)):
                toks = dc.rle_tokens(piece)
                assert dc.expand(toks) == piece, (e["name"], sm)
                assert all(t[0] == "L" or (t[2] == 1 and 3 <= t[1] <= 258) for t in toks), e["name"]


def _hlit_of(tokens):
    return max([257] + [dc.token_symbol(t)[0] + 1 for t in tokens if t[0] == "M"])


def _zero_runs(used, hlit):
    """lengths of the runs of unused symbols among the first hlit lit/len symbols"""
    return [r for s, r in dc.runs_of(bytes(1 if s in used else 0 for s in range(hlit))) if s not in used]


def test_the_crafted_set_covers_every_edge_it_names():
    """asserted on the CPU, from the payloads and the restated tokens alone, before any GPU test relies on it"""
    cat = dc.enc_by_name()
    assert len(cat) == len(dc.encode_catalogue()) and all(e["why"] for e in cat.values())
    sizes = {n: len(_payload(e)) for n, e in cat.items()}
    for name, e in cat.items():
        p = _payload(e)
        runs = dc.runs_of(p)
        for end, r in e["runs"]:                                       # the run ends where the name says, and is as long
            assert (end - r + 1, r) in runs, (name, end, r)
        types = [dc.pinned_type(dc.rle_tokens(x), len(x)) for x in dc.pieces(p)]
        if e["pin"] is not None:                                       # the block types that the entry is meant to pin are pinned
            assert tuple(types) == (e["pin"] if isinstance(e["pin"], tuple) else (e["pin"],) * len(types)), (name, types)
    # frame geometry: ends -2 .. +5 around every slab boundary, from 3, 4, 5 and ~260 back; every reachable slot of lanes 0, 1, 62, 63
    for off in range(-2, 6):
        for back in (3, 4, 5):
            assert cat["slab_end%+d_back%d" % (off, back)]["runs"] == [(256 * k - 2 + off, back + 1) for k in range(1, 9)]
        far = cat["slab_end%+d_back260_odd" % off]["runs"] + cat["slab_end%+d_back260_even" % off]["runs"]
        assert sorted(end for end, _ in far) == [256 * k - 2 + off for k in range(1, 9)]
        assert all((end + 2) // 256 > (end - r + 1 + 2) // 256 for end, r in far if end + 2 >= 256)         # each starts in front of the slab it ends in (none can in slab 0)
        assert sizes["slab_end%+d_back3" % off] == 2250 and (2250 + 2 + 255) // 256 == 9
    # every (lane, slot) cell of lanes 0, 1, 62, 63 of slab 0 and of the last, partly filled slab in which a run of >= 4 can end, read off the
    # payloads: slab 0 holds positions -2 .. 253, and a run of four cannot end in front of position 3; the last slab of a payload of 2300
    # bytes is slab 8, positions 2046 .. 2299
    first, last = set(), set()
    for e in cat.values():
        n = len(_payload(e))
        for s, r in dc.runs_of(_payload(e)):
            end = s + r - 1
            if r >= 4 and end + 2 < 256:
                first.add(divmod(end + 2, 4))
            if r >= 4 and n == 2300 and end + 2 >= 256 * 8:
                last.add(divmod(end + 2 - 256 * 8, 4))
    assert first >= {(1, 1), (1, 2), (1, 3)} | {(l, q) for l in (62, 63) for q in range(4)}, sorted(first)
    assert last >= {(l, q) for l in (0, 1, 62) for q in range(4)} | {(63, 0), (63, 1)}, sorted(last)
    assert {e["runs"][0][0] for n, e in cat.items() if n.startswith("from_position_0_to")} == {3, 4, 5}
    assert all(dc.runs_of(_payload(e))[0][0] == 0 and dc.runs_of(_payload(e))[0][1] >= 4 for n, e in cat.items() if n.startswith("from_position_0"))
    assert {sizes["length_%d" % n] % 4 for n in (2250, 2251, 2252, 2253)} == {0, 1, 2, 3}
    assert {sizes["length_%d" % n] % 256 for n in range(2301, 2307)} == {253, 254, 255, 0, 1, 2}
    assert all(cat["length_%d_run_to_the_end" % n]["runs"] == [(n - 1, 5)] for n in (2250, 2251, 2252, 2253, 2301, 2302, 2303, 2304, 2305, 2306))
    # run lengths: every rem class behind 0, 1 and 2 full matches; every length symbol; nfull = 62
    toks = dc.rle_tokens(_payload(cat["run_lengths_around_258"]))
    assert [r for _, r in cat["run_lengths_around_258"]["runs"]] == [3, 4, 5, 6, 259, 260, 261, 262, 517, 518, 519, 520]
    assert {t[1] for t in toks if t[0] == "M"} >= {3, 4, 5, 258} and sum(t[0] == "M" and t[1] == 258 for t in toks) == 12
    assert {dc.token_symbol(t)[0] for t in dc.rle_tokens(_payload(cat["length_symbols_all_29"])) if t[0] == "M"} == set(range(257, 286))
    assert sum(t == ("M", 258, 1) for t in dc.rle_tokens(_payload(cat["run_16000"]))) == 62
    # the run-heavy front of the constant signal: 499 zero key bytes and 1999 zero data bytes, then plain slabs; one of a pair holds a run after all
    front = dc.runs_of(_payload(cat["const2000_plain_aux"]))
    assert sorted(r for _, r in front)[-2:] == [499, 1999] and cat["const2000_plain_aux"]["head"] > 2550
    end, r = cat["const2000_run_in_a_plain_pair"]["runs"][0]
    gs = (len(dc.enc_hdr(cat["const2000_plain_aux"])) + 12 + 500 + 2 + 255) // 256          # run_heavy_front() in slabs
    assert (end + 2) // 256 >= gs + 1 and list(dc.slab_token_counts(_payload(cat["const2000_run_in_a_plain_pair"])))[-1] == (end + 2) // 256
    assert max(r for _, r in dc.runs_of(_payload(cat["const2000_run_from_the_front"]))) == 2299
    # the token list: the general slabs' tokens exceed the list in S.freq (fused) and all of the staged list; no slab alone does; the
    # straddle: no set of leading slabs ends exactly on entry 640
    for name in ("list_8k_run_in_every_slab", "list_16k_run_in_every_slab", "poolb_list_ok_dynamic"):
        cnt = dc.slab_token_counts(_payload(cat[name]))
        assert sum(cnt.values()) > cat[name]["list_over"] and max(cnt.values()) < dc.DEFL2_LIST_CAP, (name, sum(cnt.values()))
        assert dc.DEFL2_LIST_CAP not in np.cumsum(list(cnt.values())).tolist()
    alone = [e for e in cat.values() if e.get("listed")]
    assert len(alone) == 64 and all(sum(dc.slab_token_counts(_payload(e)).values()) <= dc.DEFL2_LIST_CAP for e in alone)
    assert {e["runs"][1][0] for e in alone} == {256 * k - 2 + off for k in range(1, 9) for off in range(-2, 6)}
    assert sizes["list_8k_run_in_every_slab"] == 8192 and sizes["list_16k_run_in_every_slab"] == sizes["poolb_list_ok_dynamic"] == 16384
    assert dc.STAGED_WF_AT == 2960 and dc.LIST_CAP_STAGED == 6432
    cnt = dc.slab_token_counts(_payload(cat["poolb_list_ok_dynamic"]))
    listb_words = ((sum(cnt.values()) - dc.DEFL2_LIST_CAP + 7) >> 3) << 2
    bits = dc.dyn_upper(dc.rle_tokens(_payload(cat["poolb_list_ok_dynamic"])))
    assert sum(cnt.values()) <= dc.LIST_CAP_STAGED and ((80 + bits + 15 + 31) >> 5) - 2 + 4 <= dc.STAGED_WF_AT - listb_words       # list_ok, whatever the code
    toks = dc.rle_tokens(_payload(cat["list_16k_run_in_every_slab"]))
    assert dc.huffman_body_bits(toks) // 32 > dc.DEFL2_LISTB_MIN                               # !list_ok, whatever the code
    # code lengths and header
    f = dc.token_freq(dc.rle_tokens(_payload(cat["cl14_two_bytes_and_rares"])))
    assert 8192 < sum(f) <= 16384 and max(dc.shannon_lengths(f)) == 14            # (the head's u64 blob length is a run in every record)
    x = dc.pieces(_payload(cat["cl15_later_block"]))[1]
    f = dc.token_freq(dc.rle_tokens(x))
    assert sum(f) == 16385 and max(dc.shannon_lengths(f)) == 15 and max(r for _, r in dc.runs_of(x)) < 4
    f = dc.token_freq(dc.rle_tokens(_payload(cat["all_286_symbols"])))
    assert all(f) and len(f) == 286
    for name, e in cat.items():
        if "zero_runs" in e:
            toks = dc.rle_tokens(_payload(e))
            used = {s for s, n in enumerate(dc.token_freq(toks)) if n}
            zr = _zero_runs(used, _hlit_of(toks))
            assert all(g in zr for g in e["zero_runs"]) and zr[0] == 31 and set(range(1, 32)).isdisjoint(used), (name, zr)
        if "repeat" in e:
            f = dc.token_freq(dc.rle_tokens(_payload(e)))
            assert len(set(f[0x80:0x80 + e["repeat"]])) == 1 and f[0x80] > 0 and f[0x7F] == 0 and f[0x80 + e["repeat"]] == 0, name
    assert {e["repeat"] for e in cat.values() if "repeat" in e} == {4, 7, 8, 10}
    assert {g for e in cat.values() for g in e.get("zero_runs", ())} == {138, 139, 140, 10, 11, 2, 3}
    assert _hlit_of(dc.rle_tokens(_payload(cat["hlit_286_only_match_258"]))) == 286
    assert max(t[1] for t in dc.rle_tokens(_payload(cat["no_match_behind_the_head"])) if t[0] == "M") <= 10      # the head's zero runs only
    # block choice and block edges
    assert sizes["shortest_record"] == 51 and sizes["payload_100"] == 100 and sizes["payload_300"] == 300
    assert all(sizes["payload_%d" % n] == n for n in (16383, 16384, 16385, 16386, 16387, 32768, 32769))
    p = _payload(cat["run_3_before_to_3_behind_the_cut"])
    assert (16381, 6) in dc.runs_of(p) and dc.rle_tokens(dc.pieces(p)[0])[-3:] == [("L", p[16381])] * 3 == dc.rle_tokens(dc.pieces(p)[1])[:3]
    p = _payload(cat["run_600_across_the_cut"])
    assert dc.rle_tokens(dc.pieces(p)[0])[-3:] == [("L", p[16084]), ("M", 258, 1), ("M", 41, 1)] and dc.rle_tokens(dc.pieces(p)[1])[:3] == [("L", p[16084]), ("M", 258, 1), ("M", 41, 1)]
    # the stored blocks: for the random entries the dynamic block's floor (dyn_lower) and the fixed block are no smaller than the stored
    # one; for the flat block even the optimal Huffman BODY alone is larger
    for name, k in (("random_with_three_runs", 0), ("stored_then_dynamic", 0), ("dynamic_then_stored", 1)):
        x = dc.pieces(_payload(cat[name]))[k]
        toks = dc.rle_tokens(x)
        assert dc.stored_bits(6, len(x)) <= min(dc.dyn_lower(toks), dc.fixed_bits(toks)), name
    # ... and the stored blocks that a fixed block without its length extra bits would seem to beat
    for name in ("fixed_near_stored",):
        e = cat[name]
        toks = dc.rle_tokens(_payload(e))
        extra = sum(dc.token_symbol(t)[1] for t in toks)
        sto, fix = dc.stored_bits(0, len(_payload(e))), dc.fixed_bits(toks)
        assert extra == e["near_fixed"] >= 4 and sto < fix < sto + extra and fix - extra < sto, name
    x = dc.pieces(_payload(cat["dynamic_then_stored"]))[1]
    assert dc.huffman_body_bits(dc.rle_tokens(x)) > dc.stored_bits(6, len(x))


def _families():
    fam = {}
    for e in dc.encode_catalogue():
        fam.setdefault(dc.enc_family(e["name"]), []).append(e)
    return fam


def test_docs_list_every_family_of_encoder_entries():
    """docs/codecs.md has one table row per family of entries (the names of one loop of the catalogue, numbers written #):
    | `family` | entries | payload bytes lo .. hi | what its first entry reaches |"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "docs", "codecs.md"), encoding="utf-8").read()
    rows = {m.group(1): m.groups()[1:] for m in re.finditer(r"^\| `([\w#]+)` \| (\d+) \| (\d+) \.\. (\d+) B \| (.*) \|$", text, re.M)}
    fam = _families()
    for name, ents in fam.items():
        sizes = [len(_payload(e)) for e in ents]
        assert rows.get(name) == (str(len(ents)), str(min(sizes)), str(max(sizes)), ents[0]["why"]), name
    assert len(rows) == len(fam) < 60


# ---------------------------------------------------------------- what every record is held to
_CHECKED = {}                     # stream -> what its blocks showed (fused and stream send the same bytes: checked once)


def _check_dynamic(b, toks, where):
    ll, f = b.litlens, dc.token_freq(toks)
    assert max(ll) <= 15 and sum(1 << (15 - l) for l in ll if l) == 32768, where                        # Kraft sum exactly 1
    assert all(s < len(ll) and ll[s] for s in range(286) if f[s]), where                                # a code for every symbol in use, 256 among them
    side = sum(dc.token_symbol(t)[1] + 1 for t in toks if t[0] == "M")
    body = sum(f[s] * ll[s] for s in range(len(ll))) - ll[256] + side
    assert body == b.end_bit - b.tokens_at - ll[256], where
    assert body <= dc.shannon_body_bits(toks), (where, body, dc.shannon_body_bits(toks))
    assert b.dlens == [1, 1] and b.hdist == 2, where
    assert b.hlit == max([257] + [s + 1 for s in range(len(ll)) if ll[s]]) == len(ll), where
    want = dc.cl_rle(ll + [1, 1])
    assert b.entries == want, where
    ca, cb = dc.cl_cost(want, dc.CLA_LENS), dc.cl_cost(want, dc.CLB_LENS)
    use_a = ca is not None and ca <= cb                                                                 # A wins ties; A lacks 14 and 15
    assert (b.cll, b.hclen) == ((dc.CLA_LENS, 18) if use_a else (dc.CLB_LENS, 19)), (where, ca, cb)
    assert use_a or max(ll) >= 14 or cb < ca, where
    return {"A" if use_a else "B"} | ({"tie"} if ca == cb else set())


def _check_record(name, rec, payload, route, observed=None):
    """-> (block types, code-length codes, code-length entries) of the record"""
    where = (name, route)
    (sz,) = struct.unpack_from("<Q", rec, 0)
    assert sz == len(rec) - 8, where
    stream = rec[8:]
    key = (payload, stream)
    if key in _CHECKED:
        return _CHECKED[key]
    assert stream[:2] == b"\x78\x9c" and dc.referee(stream) == payload, (where, ZV)
    p = dc.parse_blocks(stream)
    assert p.trailing == b"" and p.adler == zlib.adler32(payload) and p.data == payload, where
    want = dc.pieces(payload)
    assert [b.data for b in p.blocks] == want and [b.bfinal for b in p.blocks] == [0] * (len(want) - 1) + [1], where
    types, codes, entries = [], set(), set()
    for k, (b, piece) in enumerate(zip(p.blocks, want)):
        at = where + (k,)
        toks = dc.rle_tokens(piece)
        chosen = b.end_bit - b.first_bit
        fix, sto, up = dc.fixed_bits(toks), dc.stored_bits(b.first_bit, len(piece)), dc.dyn_upper(toks)
        if b.btype == 0:
            assert chosen == sto and b.pad == 0 and chosen <= fix, (at, chosen, fix)
        else:
            assert b.tokens == toks, (at, next((i, x, y) for i, (x, y) in enumerate(zip(b.tokens + [None], toks + [None])) if x != y))
            if b.btype == 1:
                assert chosen == fix and chosen < sto, (at, chosen, sto)
            else:
                assert chosen <= fix and chosen < sto, (at, chosen, fix, sto)
                assert chosen <= dc.dyn_upper(toks, b.hlit), (at, chosen)
                codes |= _check_dynamic(b, toks, at)
                entries |= set(b.entries)
        assert chosen <= up, (at, chosen, up)
        pin = dc.pinned_type(toks, len(piece))
        assert pin is None or b.btype == pin, (at, b.btype, pin)
        assert observed is None or b.btype == observed, (at, b.btype, "the entry no longer reaches the block type it was made for")
        types.append(b.btype)
    _CHECKED[key] = (types, codes, entries)
    return _CHECKED[key]


# the classes that every route must have produced somewhere in the catalogue: the three block types; both static code-length codes, and a
# sequence that costs the same under both ("tie": A wins); the code-length entries
ENTRY_CLASSES = {(16, 0), (16, 3), (17, 0), (17, 7), (18, 0), (18, 127)}      # 16 x 3 and x 6, 17 x 3 and x 10, 18 x 11 and x 138


def _check_route(ents, recs, route, sm=1):
    assert len(recs) == len(ents)
    types, codes, entries = set(), set(), set()
    for e, rec in zip(ents, recs):
        t, c, en = _check_record(e["name"], rec, _payload(e, sm), route, e.get("observed") if sm == 1 else None)
        types |= set(t)
        codes |= c
        entries |= en
    print("%s: %d records, block types %s, code-length codes %s, classes missing %s" % (route, len(recs), sorted(types), sorted(codes), sorted(ENTRY_CLASSES - entries)))
    return types, codes, entries


# ---------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def press():
    from slow5tools_amd import _lib, press as p
    _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
    return p


@contextlib.contextmanager
def fused_tier2(value):
    from slow5tools_amd import _lib
    L = _lib.lib()
    try:
        _lib.check(L.s5gpu_set_option(b"fused_tier2", value), "s5gpu_set_option")
        yield
    finally:
        _lib.check(L.s5gpu_set_option(b"fused_tier2", 0), "s5gpu_set_option")


def _group(lo, hi, sm=1, room=0):
    return [e for e in dc.encode_catalogue() if lo < len(_payload(e, sm)) + room <= hi]


def _device_batch(press, ents, cap, sm=1):
    sigs = [np.asarray(e["signal"], dtype=np.int16) for e in ents]
    hdrs = [dc.enc_hdr(e) for e in ents]
    b = press.DeviceBatch([len(s) for s in sigs], hdr_len=[len(h) for h in hdrs], aux_len=[len(e["aux"]) for e in ents], sig_method=sm, lds_payload_cap=cap)
    b.upload(sigs, hdrs, [e["aux"] for e in ents])
    return b


def _fused_groups():
    narrow, wide = _group(0, NARROW), _group(NARROW, dc.BLOCK)
    assert len(narrow) > 100 and 5 <= len(wide) <= 12 and len(narrow) + len(wide) + len(_group(dc.BLOCK, 1 << 20)) == len(dc.encode_catalogue())
    return ((narrow, NARROW), (wide, dc.BLOCK))


def _require(got, classes=ENTRY_CLASSES, types=(0, 1, 2), codes=("A", "B", "tie")):
    t, c, en = got
    assert t >= set(types), sorted(t)
    assert c >= set(codes), sorted(c)
    assert en >= classes, sorted(classes - en)


@pytest.mark.gpu
def test_route_fused(press):
    """encode(): the entries of up to 8192 bytes in one batch with that budget (the uint32_t kernels), the ones of up to one block in a
    second with 16384 (uint64_t); nothing on the overflow list"""
    got = [set(), set(), set()]
    for ents, cap in _fused_groups():
        b = _device_batch(press, ents, cap)
        assert b.tot["max_payload"] > NARROW or cap == NARROW              # (else fused_cap() clips the budget to the narrow kernels')
        b.encode()
        recs = b.records()
        assert int(b.ovf[0].item()) == 0
        for g, x in zip(got, _check_route(ents, recs, "fused %d" % cap)):
            g |= x
    _require(got)


@pytest.mark.gpu
def test_route_stream(press):
    """encode_stream(): the same two batches through the single-pass kernels; every record byte for byte the one encode() leaves in its
    slot"""
    got = [set(), set(), set()]
    for ents, cap in _fused_groups():
        b = _device_batch(press, ents, cap)
        b.encode_stream()
        recs = b.stream_records(range(len(ents)))
        assert b.stream_ok()
        for g, x in zip(got, _check_route(ents, recs, "stream %d" % cap)):
            g |= x
        b.encode()
        assert b.records() == recs
    _require(got)


@pytest.mark.gpu
def test_route_parked(press):
    """pack_parked() + deflate_parked(): every entry, the small ones too, through deflate_block2<2, 256> — the token list's second pool,
    blocks behind blocks"""
    ents = dc.encode_catalogue()
    b = _device_batch(press, ents, 0)
    b.pack_parked()
    b.deflate_parked()
    _require(_check_route(ents, b.records(), "parked"))


@pytest.mark.gpu
def test_route_overflow_list(press):
    """encode() with a budget below the shortest payload: the fused launch declines every read, k_deflate_staged takes them from the
    overflow list"""
    ents = dc.encode_catalogue()
    with fused_tier2(0):
        b = _device_batch(press, ents, 48)
        b.encode()
        recs = b.records()
        assert int(b.ovf[0].item()) == len(ents)
    _require(_check_route(ents, recs, "overflow"))


@pytest.mark.gpu
def test_route_second_fused_launch(press):
    """option fused_tier2: a first fused launch with a budget of 2048 bytes, a second (four workgroups per CU) with one block, the
    staged kernels for the entries of more than one block — which are the only ones on the overflow list"""
    ents = dc.encode_catalogue()
    with fused_tier2(dc.BLOCK):
        b = _device_batch(press, ents, 2048)
        b.encode()
        recs = b.records()
        assert int(b.ovf[0].item()) == len(_group(dc.BLOCK, 1 << 20))
    assert len(_group(0, 2048)) >= 10 and len(_group(2048, dc.BLOCK)) >= 100
    _require(_check_route(ents, recs, "tier2"))


@pytest.mark.gpu
def test_route_host(press):
    """press.encode_records: what s5gpu_encode_batch makes of the whole catalogue in one call"""
    ents = dc.encode_catalogue()
    recs = press.encode_records([np.asarray(e["signal"], dtype=np.int16) for e in ents], [dc.enc_hdr(e) for e in ents], [e["aux"] for e in ents])
    _require(_check_route(ents, recs, "host"))


@pytest.mark.gpu
def test_route_exzd(press):
    """the entries of up to 8192 bytes once more with SIG_EX_ZD: the EXZD instantiations of the fused and the single-pass kernel build
    another blob in front of the same aux bytes; the payload is the oracle's rec_pack(r, 2)"""
    ents = _group(0, NARROW, sm=2, room=64)
    assert len(ents) > 100
    b = _device_batch(press, ents, NARROW, sm=2)
    b.encode()
    recs = b.records()
    assert int(b.ovf[0].item()) == 0
    got = _check_route(ents, recs, "exzd fused", sm=2)
    b.encode_stream()
    assert b.stream_records(range(len(ents))) == recs and b.stream_ok()
    _require(got)


@pytest.mark.gpu
def test_every_route_sends_the_same_tokens(press):
    """the token lists are the restated ones on every route (asserted record by record above), so they are the same on all of them; here
    the stronger statement for the staged routes: parked, overflow list and host give byte-identical records"""
    ents = dc.encode_catalogue()
    b = _device_batch(press, ents, 0)
    b.pack_parked()
    b.deflate_parked()
    parked = b.records()
    with fused_tier2(0):
        b2 = _device_batch(press, ents, 48)
        b2.encode()
        assert b2.records() == parked
    big = [k for k, e in enumerate(ents) if len(_payload(e)) > dc.BLOCK]
    host = press.encode_records([np.asarray(e["signal"], dtype=np.int16) for e in ents], [dc.enc_hdr(e) for e in ents], [e["aux"] for e in ents])
    assert [host[k] for k in big] == [parked[k] for k in big]
