"""Every route of the zstd frame decoder on hand-made frames (tests/zstd_craft.py).  Valid frames carry the content the builder got
by executing its own sequences; libzstd is the referee of what is a frame at all.  The CPU tests pin the catalogue and the restated
decoder (oracle/zstd_dec.c) on libzstd; the GPU tests put the same frames, seeded mutants of them and crafted record frames through
the device decoder (csrc/zstd_dev.h), once with the weights pass (k_zstd_weights) forced on and once without it."""
import functools

import numpy as np
import pytest

import oracle_bind as ob
import zstd_craft as zc
from test_oracle_golden import needs_zstd

REJECT_CAP = 1 << 20            # room offered to a decoder for a frame that must be refused (no such frame says more)


def _cap(expected):
    return len(expected) if expected is not None else REJECT_CAP


def test_catalogue_covers_every_route():
    """nobody drops a row quietly: the routes taken by the valid frames are exactly the routes named"""
    took = set()
    for _, _, expected, tags in zc.CATALOGUE:
        if expected is not None:
            took |= tags
    assert took == set(zc.ROUTES), (sorted(set(zc.ROUTES) - took), sorted(took - set(zc.ROUTES)))
    assert len(zc.CATALOGUE) > 64 and len({name for name, _, _, _ in zc.CATALOGUE}) == len(zc.CATALOGUE)
    assert max(len(e) for _, _, e, _ in zc.CATALOGUE if e is not None) <= 8 << 20


def test_restated_decoder_on_the_catalogue():
    """oracle/zstd_dec.c: the builder's bytes for every valid frame, a refusal for every other (needs no libzstd)"""
    for name, data, expected, _ in zc.CATALOGUE:
        assert ob.zstd_restated_decompress(data, _cap(expected)) == expected, name


@needs_zstd
def test_libzstd_on_the_catalogue():
    """libzstd decodes every valid frame to the builder's bytes and refuses every invalid one — but for the rows tagged STRICTER, which
    the format refuses and libzstd 1.4.8 lets pass (docs/codecs.md, differences from libzstd): nothing is asked of libzstd there"""
    for name, data, expected, tags in zc.CATALOGUE:
        if zc.STRICTER in tags:
            continue
        assert ob.zstd_decompress(data, _cap(expected)) == expected, name


# ---- mutants ----
MUTANT_SEED = 5
MUTANT_LARGEST_SOURCE = 300000   # content of the largest frame that is mutated (the multi-megabyte frames stay out: test budget)


def _huffman_ranges(data):
    """byte ranges of the Huffman-coded literals sections of a crafted frame"""
    out, p = [], 5 + (0 if (data[4] >> 5) & 1 else 1) + {0: (data[4] >> 5) & 1, 1: 2, 2: 4, 3: 8}[data[4] >> 6]
    while p + 3 <= len(data):
        bh = int.from_bytes(data[p:p + 3], "little")
        p += 3
        typ, size = (bh >> 1) & 3, bh >> 3
        if typ == 2 and data[p] & 3 >= 2:
            sf = (data[p] >> 2) & 3
            bits, hl = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
            csize = (int.from_bytes(data[p:p + 5], "little") >> (4 + bits)) & ((1 << bits) - 1)
            out.append((p + hl, p + hl + csize))
        p += size if typ != 1 else 1
        if bh & 1:
            break
    return out


@functools.lru_cache(maxsize=None)
def mutants():
    """(source name, frame, room, lax) — from every valid catalogue frame up to MUTANT_LARGEST_SOURCE bytes of content: three copies
    with 1, 2 and 3 bytes changed and one cut short.  Dropped, by a property of the mutant's own bytes (zstd_craft.walk): a dictionary-ID
    bit in the frame header (the device refuses dictionaries, libzstd without one ignores the ID), a declared content size above 1 MiB
    (test budget), and what docs/codecs.md lists as refused here but accepted by libzstd 1.4.8 — a Block_Size above 128 KiB, a sequence
    count of zero in its long form, reserved bits in a modes byte.  `lax`: a changed byte lies inside Huffman-coded literals, where
    libzstd's double-symbol decoder lets the last symbol of a stream overrun; such a mutant may be refused here and accepted there."""
    rng = np.random.default_rng(MUTANT_SEED)
    out = []
    for name, data, expected, _ in zc.CATALOGUE:
        if expected is None or len(expected) > MUTANT_LARGEST_SOURCE:
            continue
        huf = _huffman_ranges(data)
        for k in range(4):
            g, lax = bytearray(data), False
            if k < 3:
                for pos in rng.integers(0, len(g), k + 1):
                    g[pos] = rng.integers(0, 256)
                    lax = lax or any(a <= pos < b for a, b in huf)
            else:
                g = g[:int(rng.integers(1, len(g)))]
            g = bytes(g)
            w = zc.walk(g)
            if g == data or (w["fhd"] is not None and w["fhd"] & 3) or (w["fcs"] is not None and w["fcs"] > 1 << 20) or w["largest_block"] > 131072:
                continue
            if any((nbytes > 1 and nseq == 0) or (nseq and modes is not None and modes & 3) for nbytes, nseq, modes in w["blocks"]):
                continue
            out.append((name, g, max(len(expected), w["fcs"] or 0) + 1024, lax))
    return out


@functools.lru_cache(maxsize=None)
def mutant_answers():
    """libzstd's answer for every mutant (None: refused), with the proof that the set is not one-sided"""
    ref = [ob.zstd_decompress(g, cap) for _, g, cap, _ in mutants()]
    n_ok = sum(r is not None for r in ref)
    assert n_ok >= 20 and len(ref) - n_ok >= 20 and 200 <= len(ref) <= 600, (n_ok, len(ref))
    return ref


@needs_zstd
def test_restated_decoder_and_libzstd_agree_on_mutants():
    for (name, g, cap, lax), ref in zip(mutants(), mutant_answers()):
        mine = ob.zstd_restated_decompress(g, cap)
        if mine is not None:
            assert mine == ref, name
        elif not lax:
            assert ref is None, name


# ---- crafted frames around record payloads ----
def runs_as_sequences(payload, min_run=5):
    """(literals, sequences): every run of at least min_run equal bytes is one literal and a match at offset 1 behind it"""
    lits, seqs, i, pend, n = bytearray(), [], 0, 0, len(payload)
    while i < n:
        j = i
        while j < n and payload[j] == payload[i]:
            j += 1
        if j - i >= min_run:
            lits.append(payload[i])
            seqs.append((pend + 1, j - i - 1, 4))                     # Offset_Value 4: offset 1, whatever the history
            pend = 0
        else:
            lits += payload[i:j]
            pend += j - i
        i = j
    return bytes(lits), seqs


def record_frames(payload):
    cuts = [0, 1, 8, 71, 1000, 4097]
    pieces = [payload[a:b] for a, b in zip(cuts, cuts[1:] + [len(payload)]) if a < len(payload)] or [b""]
    lits, seqs = runs_as_sequences(payload)
    lraw = lambda x: zc.lraw(x, sf=None if x else 1)                  # (no literals at all: two header bytes, a compressed block has at least 3)
    return [zc.frame([zc.raw(x) for x in pieces]),
            zc.frame([zc.comp(lraw(payload))]),
            zc.frame([zc.comp(lraw(lits), seqs, modes=(("fse", 6), "rle", "predef"))]),
            zc.frame([zc.raw(x) for x in pieces], single_segment=False, fcs=0),
            zc.frame([zc.comp(lraw(lits), seqs, modes=("predef", "rle", ("fse", 6)))], single_segment=False, fcs=0)]


def test_runs_as_sequences_rebuild_the_payload():
    """the record frames hold what they are said to hold (CPU: the builder's own execution, the restated decoder, libzstd when present)"""
    rng = np.random.default_rng(3)
    for n in (0, 1, 40, 3000):
        p = bytes(np.repeat(rng.integers(0, 256, n // 4 + 1, dtype=np.uint8), rng.integers(1, 12, n // 4 + 1))[:n])
        for f in record_frames(p):
            assert f.expected == p and ob.zstd_restated_decompress(f.data, len(p)) == p
            if ob.zstd_ref() is not None:
                assert ob.zstd_decompress(f.data, len(p)) == p


# ---- the device ----
@pytest.mark.gpu
class TestDevice:
    @pytest.fixture(scope="class")
    def press(self):
        from slow5tools_amd import _lib, press as p
        _lib.check(_lib.lib().s5gpu_init(0), "s5gpu_init")
        return p

    @pytest.fixture(autouse=True, params=["weights-pass", "in-wave"])
    def first_tree(self, request, press):
        """every test of this class twice: with the pass that decodes the first tree description of every frame a frame per lane
        (k_zstd_weights, by default from 256 frames on) forced on for any batch, and without it (the frame's wave walks the chain itself)"""
        from slow5tools_amd import _lib
        L = _lib.lib()
        _lib.check(L.s5gpu_set_option(b"zstd_pre_min", 1 if request.param == "weights-pass" else 0))
        yield request.param
        _lib.check(L.s5gpu_set_option(b"zstd_pre_min", 256))

    @staticmethod
    def solo(frames):
        from test_zstd import zstd_solo
        return zstd_solo(frames)

    def test_valid_catalogue_frames_decode_to_the_expected_bytes(self, press):
        rows = [r for r in zc.CATALOGUE if r[2] is not None]
        assert len(rows) > 64                                              # full waves of the weights pass and a partial one
        rc, res, st = self.solo([r[1] for r in rows])
        for (name, _, expected, _), r, s in zip(rows, res, st):
            assert s == 0 and r == expected, (name, s)
        assert rc == 0
        order = np.random.default_rng(9).permutation(len(rows))
        rc2, res2, st2 = self.solo([rows[i][1] for i in order])
        assert rc2 == 0 and [st2[k] for k in np.argsort(order)] == st and [res2[k] for k in np.argsort(order)] == res

    def test_whole_catalogue_in_one_batch_and_shuffled(self, press):
        frames = [r[1] for r in zc.CATALOGUE]
        rc, res, st = self.solo(frames)
        for (name, _, expected, _), r, s in zip(zc.CATALOGUE, res, st):
            if expected is None:
                assert s != 0 and r is None, (name, s)
            else:
                assert s == 0 and r == expected, (name, s)
        assert rc != 0
        order = np.random.default_rng(10).permutation(len(frames))
        rc2, res2, st2 = self.solo([frames[i] for i in order])
        back = np.argsort(order)
        assert rc2 == rc and [st2[k] for k in back] == st and [res2[k] for k in back] == res

    @pytest.mark.parametrize("sig_name", ["svb-zd", "ex-zd"])
    def test_crafted_frames_around_record_payloads(self, press, sig_name):
        sm = {"svb-zd": press.SIG_SVB_ZD, "ex-zd": press.SIG_EX_ZD}[sig_name]
        rng = np.random.default_rng(61)
        sigs = [(500 + np.cumsum(rng.integers(-15, 16, n)) % 300).astype(np.int16) for n in (0, 1, 5, 400, 4000)]
        sigs.append(np.repeat(rng.integers(300, 700, 100), rng.integers(1, 80, 100))[:4000].astype(np.int16))   # plateaus: long runs in the payload
        hdrs = [press.pack_hdr(b"read_%06d" % i, i % 3, 8192.0, 23.0, 1467.61, 4000.0) for i in range(len(sigs))]
        auxs = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in (0, 3, 40, 0, 17, 9)]
        raw = press.encode_records(sigs, hdrs, auxs, press.REC_NONE, sm)
        frames, src = [], []
        for i, r in enumerate(raw):
            for f in record_frames(r[8:]):
                assert f.expected == r[8:]
                frames.append(f.data)
                src.append(i)
        assert any(f[4] >> 5 == 0 for f in frames)                        # one shape has no content size
        dec = press.decode_records(frames, press.REC_ZSTD, sm)
        for d, i in zip(dec, src):
            assert d["status"] == 0 and np.array_equal(d["signal"], sigs[i]) and d["aux"] == auxs[i] and d["read_id"] == b"read_%06d" % i

    def test_mutants_of_catalogue_frames_against_libzstd(self, press):
        """libzstd referees both ways: what the device accepts libzstd accepts with the same bytes, and what libzstd accepts the device
        accepts (but where mutants() says libzstd is the lax one)"""
        if ob.zstd_ref() is None:
            pytest.skip("no libzstd.so.1 in this image")
        M, ref = mutants(), mutant_answers()
        rc, res, st = self.solo([g for _, g, _, _ in M])
        for (name, g, _, lax), want, r, s in zip(M, ref, res, st):
            if s == 0:
                assert r == want, name
            else:
                assert r is None and (want is None or lax), (name, s)
