"""Hand-made Zstandard frames for the decoder tests (test infrastructure, written from RFC 8878; libzstd is the referee of what is
valid, tests/test_zstd_craft.py asks it about every frame made here).

frame(blocks, ...) turns a list of block specs into a Crafted(data, expected, tags):

  raw(data) / rle(byte, n)                 the two plain block kinds
  comp(literals, sequences, modes=...)     a compressed block: a literals spec (lraw / lrle / lhuf / ltreeless), a list of
                                           (literal length, match length, Offset_Value) triples and the mode of each of the three
                                           sequence tables: "predef", "rle", "fse" / ("fse", log) / ("fse", log, norm), "repeat"

`expected` is the content, computed here by executing the sequences (None when the builder itself sees that the frame cannot be
decoded: an offset of zero or beyond the output, literals that run out); `tags` names the routes of the decoder that the frame takes.
CATALOGUE lists (name, frame bytes, expected | None, tags): the smallest frames that take each route in ROUTES, and frames that
must be refused (expected None; the tag STRICTER marks the few that the format and this project refuse but libzstd 1.4.8 accepts).  Knobs that only make INVALID frames (reserved bits, forged sizes, damaged streams) are keyword arguments marked
"forge".

For the ENCODER's tests (tests/test_zstd_encode_craft.py) the second half of the file holds parse_frame (a frame read down to its fields, RFC 8878), the
restatement of what the device encoder must do (zenc_pieces, zenc_tokens, zenc_split) and zenc_catalogue(), the payloads that reach its edges.
"""
import collections
import os
import struct
import sys
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_zstd_seq_tables as _g   # noqa: E402  (the predefined distributions and the extra bits of the length codes)

from deflate_craft import huff_lengths   # noqa: E402

MAGIC = b"\x28\xb5\x2f\xfd"
LL_DEF, OF_DEF, ML_DEF = list(_g.LL), list(_g.OF), list(_g.ML)
LL_BITS, ML_BITS = list(_g.LL_BITS), list(_g.ML_BITS)
LL_BASE, ML_BASE = [0], [3]
for _b in LL_BITS[:-1]:
    LL_BASE.append(LL_BASE[-1] + (1 << _b))
for _b in ML_BITS[:-1]:
    ML_BASE.append(ML_BASE[-1] + (1 << _b))
assert LL_BASE[25] == 64 and LL_BASE[35] == 65536 and ML_BASE[43] == 131 and ML_BASE[52] == 65539
DEF = {"ll": (LL_DEF, 6), "of": (OF_DEF, 5), "ml": (ML_DEF, 6)}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}

Crafted = collections.namedtuple("Crafted", "data expected tags")


# ---- bit writers ----
class FwdBits:
    """least significant bit first (FSE count headers)"""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        self.acc |= v << self.n
        self.n += nb

    def done(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


class BackBits(FwdBits):
    """a stream that is READ from its last bit down: what is put last is read first, a value's top bit first; done() sets the end mark"""
    def done(self, mark=True):
        if mark:
            self.put(1, 1)
        return FwdBits.done(self)


# ---- FSE ----
class Fse:
    """decode cells of a normalised distribution (-1: "less than one"), and the encoder's view of them"""
    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, (sum(abs(c) for c in norm), size)
        step, mask = (size >> 1) + (size >> 3) + 3, size - 1
        high, cell, nxt = size - 1, [0] * size, []
        for s, c in enumerate(norm):
            if c == -1:
                cell[high] = s; high -= 1; nxt.append(1)
            else:
                nxt.append(c)
        pos = 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                cell[pos] = s
                pos = (pos + step) & mask
                while pos > high:
                    pos = (pos + step) & mask
        assert pos == 0
        self.norm, self.log, self.sym, self.nb, self.base = list(norm), log, cell, [0] * size, [0] * size
        self.cells = collections.defaultdict(list)
        for u in range(size):
            s = cell[u]
            ns = nxt[s]; nxt[s] += 1
            self.nb[u] = log - (ns.bit_length() - 1)
            self.base[u] = (ns << self.nb[u]) - size
            self.cells[s].append(u)

    @classmethod
    def rle(cls, sym):
        t = cls.__new__(cls)
        t.norm, t.log, t.sym, t.nb, t.base, t.cells = None, 0, [sym], [0], [0], {sym: [0]}
        return t

    def last_state(self, s, pick=0):
        """a state for the symbol that is decoded last (nothing is read behind it: any cell of the symbol will do)"""
        assert s in self.cells, "symbol %d is not in the table" % s
        return self.cells[s][pick % len(self.cells[s])]

    def before(self, s, nxt):
        """the state that decodes s and can move on to state nxt: (state, bits value, bits)"""
        assert s in self.cells, "symbol %d is not in the table" % s
        for u in self.cells[s]:
            if self.base[u] <= nxt < self.base[u] + (1 << self.nb[u]):
                return u, nxt - self.base[u], self.nb[u]
        raise AssertionError("no cell of %d reaches %d" % (s, nxt))


def normalise(hist, log, low=()):
    """counts -> a distribution over 1 << log cells; every symbol seen gets at least one cell; symbols in `low` are given -1"""
    size, total = 1 << log, sum(hist)
    norm = [0] * len(hist)
    for s, h in enumerate(hist):
        if h:
            norm[s] = -1 if s in low else max(1, h * size // total)
    big = max(range(len(hist)), key=lambda s: norm[s])
    norm[big] += size - sum(abs(c) for c in norm)
    assert norm[big] >= 1
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


def ncount(norm, log):
    """the count header of an FSE table (RFC 8878 4.1.1)"""
    b = FwdBits()
    b.put(log - 5, 4)
    remaining, threshold, nbits, prev0, s = (1 << log) + 1, 1 << log, log + 1, False, 0
    while remaining > 1:
        if prev0:
            n0 = 0
            while norm[s + n0] == 0:
                n0 += 1
            s += n0
            while n0 >= 3:
                b.put(3, 2); n0 -= 3
            b.put(n0, 2)
        c = norm[s]
        v, maxv = c + 1, 2 * threshold - 1 - remaining
        if v < maxv:
            b.put(v, nbits - 1)
        elif v < threshold:
            b.put(v, nbits)
        else:
            b.put(v + maxv, nbits)
        remaining -= abs(c)
        s += 1
        prev0 = c == 0
        while remaining < threshold:
            nbits -= 1; threshold >>= 1
    assert remaining == 1 and s == len(norm)
    return b.done()


def fse_two_states(t, syms):
    """symbols through two interleaved states (the Huffman weights; RFC 8878 4.2.1.2): even places on the first state"""
    n = len(syms)
    assert n >= 2
    st = [0] * n
    st[n - 1], st[n - 2] = t.last_state(syms[n - 1]), t.last_state(syms[n - 2])
    b = BackBits()
    for k in range(n - 3, -1, -1):
        st[k], v, nb = t.before(syms[k], st[k + 2])
        b.put(v, nb)
    b.put(st[1], t.log)
    b.put(st[0], t.log)
    return b.done()


# ---- Huffman ----
class Huf:
    """weights[s] (0: absent) of every symbol up to the last one present; the last weight is the implied one"""
    def __init__(self, weights):
        w = list(weights)
        while w and w[-1] == 0:
            w.pop()
        total = sum(1 << (x - 1) for x in w if x)
        self.weights, self.maxbits = w, total.bit_length() - 1
        self.complete = total == 1 << self.maxbits and len([x for x in w if x]) >= 2
        at, self.code = 0, {}
        for r in range(1, self.maxbits + 2):
            for s, x in enumerate(w):
                if x == r:
                    self.code[s] = (at >> (r - 1), self.maxbits + 1 - r)
                    at += 1 << (r - 1)

    @classmethod
    def for_data(cls, data, limit=11):
        hist = [0] * 256
        for x in data:
            hist[x] += 1
        if sum(1 for h in hist if h) < 2:
            hist[(data[0] + 1) % 256 if data else 1] += 1
            if not data:
                hist[0] += 1
        lens = huff_lengths(hist, limit)
        m = max(lens)
        return cls([m + 1 - l if l else 0 for l in lens])

    def stream(self, data):
        b = BackBits()
        for x in reversed(data):
            c, nb = self.code[x]
            b.put(c, nb)
        return b.done()

    def description(self, form):
        listed = self.weights[:-1]
        if form == "direct":
            assert 1 <= len(listed) <= 128
            nib = listed + [0]
            return bytes([127 + len(listed)]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(listed), 2))
        assert form == "fse"
        hist = [0] * (max(listed) + 1)
        for x in listed:
            hist[x] += 1
        assert sum(1 for h in hist if h) >= 2, "one weight value only: not FSE-codable"
        norm = normalise(hist, 6)
        body = ncount(norm, 6) + fse_two_states(Fse(norm, 6), listed)
        assert len(body) < 128
        return bytes([len(body)]) + body


# ---- block and literal specs ----
def raw(data):
    return {"kind": "raw", "data": bytes(data)}


def forged(btype, size, body=b""):
    """a block header written as told (type 0..3, any size) and whatever bytes follow it: for frames that must be refused"""
    return {"kind": "forged", "type": btype, "size": size, "body": bytes(body)}


def rle(byte, n):
    return {"kind": "rle", "byte": byte, "n": n}


def comp(lits, seqs=(), modes=("predef", "predef", "predef"), **forge):
    """forge: nseq_bytes (the count in 1 / 2 / 3 bytes whatever its value), rle_sym={"ll": 40}, stream=callable on the sequence bit stream,
    cover={"ll": codes} (not a forgery: codes an FSE table made here holds beyond the block's own), spare_bits=n (zero bits left unread), tail=bytes behind the section, modes_low=reserved bits, size=block size written"""
    return {"kind": "comp", "lits": lits, "seqs": list(seqs), "modes": tuple(modes), "forge": forge}


def lraw(data, sf=None):
    return {"kind": "raw", "data": bytes(data), "sf": sf}


def lrle(byte, n, sf=None):
    return {"kind": "rle", "data": bytes([byte]) * n, "sf": sf}


def lhuf(data, streams=1, sf=None, weights=None, desc="direct", **forge):
    """forge: desc_bytes (a tree description written instead of the one in use), stream=callable on each Huffman stream"""
    return {"kind": "huf", "data": bytes(data), "streams": streams, "sf": sf, "weights": weights, "desc": desc, "forge": forge}


def ltreeless(data, streams=1, sf=None):
    return {"kind": "treeless", "data": bytes(data), "streams": streams, "sf": sf, "forge": {}}


def _lit_header(kind, lsize, csize, streams, sf):
    typ = {"raw": 0, "rle": 1, "huf": 2, "treeless": 3}[kind]
    if typ < 2:
        if sf is None:
            sf = 2 * (lsize & 1) if lsize < 32 else 1 if lsize < 4096 else 3
        if sf in (0, 2):                                    # one byte: the format is bit 2 alone, bit 3 is the size's lowest bit
            assert lsize < 32 and sf == 2 * (lsize & 1)
            return bytes([typ | (lsize << 3)]), sf
        v = typ | (sf << 2) | (lsize << 4)
        assert lsize < (1 << (12 if sf == 1 else 20))
        return v.to_bytes(2 if sf == 1 else 3, "little"), sf
    if sf is None:
        sf = (0 if streams == 1 else 1) if max(lsize, csize) < 1024 else 2 if max(lsize, csize) < 16384 else 3
    assert (sf == 0) == (streams == 1)
    bits = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert lsize < (1 << bits) and csize < (1 << bits), (lsize, csize, sf)
    v = typ | (sf << 2) | (lsize << 4) | (csize << (4 + bits))
    return v.to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[sf], "little"), sf


def _code_of(base, v):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c


class _Builder:
    def __init__(self):
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.huf = None
        self.tab = {"ll": None, "of": None, "ml": None}     # (Fse, how it was made)
        self.tags = set()
        self.ok = True                                      # the frame can be decoded, as far as the builder can tell
        self.seen_comp = 0

    # -- literals section --
    def literals(self, L, tree_age):
        kind, data, n = L["kind"], L["data"], len(L["data"])
        if kind in ("raw", "rle"):
            hdr, sf = _lit_header(kind, n, 0, 1, L["sf"])
            self.tags.add("lit_%s_sf%d" % (kind, sf))
            return hdr + (data if kind == "raw" else data[:1] or b"\0")
        fg = L["forge"]
        if kind == "huf":
            huf = Huf(L["weights"]) if L["weights"] is not None else Huf.for_data(data)
            desc = fg["desc_bytes"] if "desc_bytes" in fg else huf.description(L["desc"])
            if "desc_bytes" in fg or not huf.complete or huf.maxbits > 11:
                self.ok = False
            else:
                self.tags.add("weights_fse" if L["desc"] == "fse" else "weights_direct_%s" % ("odd" if len(huf.weights[:-1]) & 1 else "even"))
                if huf.maxbits == 11:
                    self.tags.add("huf_maxlen_11")
            self.huf = huf
        else:
            desc = b""
            if self.huf is None:
                self.ok = False
                self.huf = Huf.for_data(data)
            else:
                self.tags.add("treeless_across_raw" if tree_age > 2 else "treeless_prev")
            huf = self.huf
        mangle = fg.get("stream", lambda s: s)
        if "stream" in fg:
            self.ok = False
        if L["streams"] == 1:
            body = mangle(huf.stream(data))
            self.tags.add("huf_1stream")
        else:
            per = (n + 3) // 4
            parts = [mangle(huf.stream(data[k * per:(k + 1) * per] if k < 3 else data[3 * per:])) for k in range(4)]
            body = b"".join(struct.pack("<H", len(x)) for x in parts[:3]) + b"".join(parts)
            if n in (6, 7, 511, 512):
                self.tags.add("huf_4stream_%d" % n)
            if n >= 8192:
                self.tags.add("huf_two_tile")
        hdr, sf = _lit_header(kind, n, len(desc) + len(body), L["streams"], L["sf"])
        self.tags.add("lit_huf_sf%d" % sf)
        return hdr + desc + body

    # -- one sequence table --
    def table(self, which, mode, codes, forge):
        name = mode if isinstance(mode, str) else mode[0]
        prev = self.tab[which]
        if name == "predef":
            t, desc = Fse(*DEF[which]), b""
        elif name == "rle":
            sym = forge.get("rle_sym", {}).get(which)
            if sym is not None:
                self.ok = False
            else:
                assert len(set(codes)) == 1, "RLE mode wants one code, got %r" % sorted(set(codes))
                sym = codes[0]
            t, desc = Fse.rle(codes[0]), bytes([sym])
        elif name == "fse":
            log = mode[1] if not isinstance(mode, str) and len(mode) > 1 else 5
            if not isinstance(mode, str) and len(mode) > 2:
                norm = list(mode[2])
            else:
                codes = list(codes) + list(forge.get("cover", {}).get(which, ()))   # codes a later block wants from this table (Repeat_Mode)
                hist = [0] * (max(codes) + 1)
                for c in codes:
                    hist[c] += 1
                if sum(1 for h in hist if h) < 2:                         # a table of one symbol is RLE's business: give it company
                    hist[0 if codes[0] else 1] += 1
                norm = normalise(hist, log)
            t, desc = Fse(norm, log), ncount(norm, log)
            if log > MAX_LOG[which]:
                self.ok = False
            elif log == MAX_LOG[which]:
                self.tags.add("%s_fse_maxlog" % which)
        else:
            assert name == "repeat"
            if prev is None:
                self.ok = False
                prev = (Fse(*DEF[which]), "predef")
            else:
                self.tags.add("%s_repeat_after_%s" % (which, prev[1]))
            return prev[0], b"", 3
        if self.ok:
            self.tags.add("%s_%s" % (which, name))
        self.tab[which] = (t, name)
        return t, desc, {"predef": 0, "rle": 1, "fse": 2}[name]

    # -- sequences section --
    def sequences(self, B, lits):
        seqs, fg = B["seqs"], B["forge"]
        n = len(seqs)
        nb = fg.get("nseq_bytes", 1 if n < 128 else 2 if n < 0x7F00 else 3)
        if nb == 1:
            head = bytes([n])
        elif nb == 2:
            head = bytes([128 + (n >> 8), n & 255])
        else:
            head = b"\xff" + struct.pack("<H", n - 0x7F00)
        if n in (0, 1, 63, 64, 65, 127, 128, 129) and "nseq_bytes" not in fg:
            self.tags.add("nseq_%d" % n)
        if n >= 0x7F00:
            self.tags.add("nseq_3byte")
        # execute: the expected bytes, and the codes
        li, first = 0, True
        coded = []
        for ll, ml, ofv in seqs:
            assert ll >= 0 and ml >= 3 and ofv >= 1
            llc, mlc, ofc = _code_of(LL_BASE, ll), _code_of(ML_BASE, ml), ofv.bit_length() - 1
            coded.append(((llc, ll - LL_BASE[llc], LL_BITS[llc]), (mlc, ml - ML_BASE[mlc], ML_BITS[mlc]), (ofc, ofv - (1 << ofc), ofc)))
            if llc == 35 and mlc == 52:
                self.tags.add("ll_code_35_ml_code_52")
            if ofc in (20, 21, 22):
                self.tags.add("of_code_%d" % ofc)
            if ofv > 3:
                off = ofv - 3
                self.rep = [off, self.rep[0], self.rep[1]]
            else:
                idx = ofv - 1 + (ll == 0)
                self.tags.add("rep%d_ll%s" % (ofv, "0" if ll == 0 else "pos"))
                if first and self.seen_comp:
                    self.tags.add("rep_across_blocks")
                if idx == 0:
                    off = self.rep[0]
                else:
                    off = self.rep[idx] if idx < 3 else self.rep[0] - 1
                    self.rep = [off, self.rep[0], self.rep[1]] if idx > 1 else [off, self.rep[0], self.rep[2]]
            first = False
            if li + ll > len(lits) or off == 0 or off > len(self.out) + ll:
                self.ok = False                                       # (still written out: the decoders have to refuse it)
                continue
            self.out += lits[li:li + ll]
            li += ll
            if off >= ml:
                self.out += self.out[len(self.out) - off:len(self.out) - off + ml]
            else:
                pat = bytes(self.out[-off:])
                self.out += (pat * (ml // off + 1))[:ml]
        self.out += lits[li:]
        if "tail" in fg or (n == 0 and nb > 1):
            self.ok = False
        if n == 0:
            return head + fg.get("tail", b"")
        if li < len(lits):
            self.tags.add("lit_leftover")
        tabs, descs, mbyte = {}, b"", fg.get("modes_low", 0)
        for k, (which, shift) in enumerate((("ll", 6), ("of", 4), ("ml", 2))):
            t, d, m = self.table(which, B["modes"][k], [c[{"ll": 0, "ml": 1, "of": 2}[which]][0] for c in coded], fg)
            tabs[which] = t
            descs += d
            mbyte |= m << shift
        if mbyte & 3:
            self.ok = False
        # the bit stream, written from the last sequence to the first
        b = BackBits()
        b.put(0, fg.get("spare_bits", 0))
        if "spare_bits" in fg or "stream" in fg:
            self.ok = False
        (llc, llx, lln), (mlc, mlx, mln), (ofc, ofx, ofn) = coded[-1]
        sl, sm, so = tabs["ll"].last_state(llc), tabs["ml"].last_state(mlc), tabs["of"].last_state(ofc)
        b.put(llx, lln); b.put(mlx, mln); b.put(ofx, ofn)
        for (llc, llx, lln), (mlc, mlx, mln), (ofc, ofx, ofn) in reversed(coded[:-1]):
            so, v, k = tabs["of"].before(ofc, so); b.put(v, k)
            sm, v, k = tabs["ml"].before(mlc, sm); b.put(v, k)
            sl, v, k = tabs["ll"].before(llc, sl); b.put(v, k)
            b.put(llx, lln); b.put(mlx, mln); b.put(ofx, ofn)
        b.put(sm, tabs["ml"].log); b.put(so, tabs["of"].log); b.put(sl, tabs["ll"].log)
        stream = fg.get("stream", lambda s: s)(b.done())
        return head + bytes([mbyte]) + descs + stream + fg.get("tail", b"")

    def block(self, B, last, tree_age):
        kind = B["kind"]
        if kind == "forged":
            self.ok = False
            return struct.pack("<I", int(last) | (B["type"] << 1) | (B["size"] << 3))[:3] + B["body"]
        if kind == "raw":
            d = B["data"]
            self.out += d
            if len(d) in (0, 1, 63, 64, 65, 131072):
                self.tags.add("raw_%d" % len(d))
            if last and not d:
                self.tags.add("raw_last_empty")
            if len(d) > 131072:
                self.ok = False
            return struct.pack("<I", int(last) | (0 << 1) | (len(d) << 3))[:3] + d
        if kind == "rle":
            n = B["n"]
            self.out += bytes([B["byte"]]) * n
            if n in (0, 1, 63, 64, 65, 131072):
                self.tags.add("rle_%d" % n)
            if last and not n:
                self.tags.add("rle_last_empty")
            if n > 131072:
                self.ok = False
            return struct.pack("<I", int(last) | (1 << 1) | (n << 3))[:3] + bytes([B["byte"]])
        L = B["lits"]
        body = self.literals(L, tree_age)
        if not L["data"]:
            self.tags.add("lit_none")
            if last and not B["seqs"]:
                self.tags.add("comp_last_empty")
        body += self.sequences(B, L["data"])
        self.seen_comp += 1
        size = B["forge"].get("size", len(body))
        if "size" in B["forge"]:
            self.ok = False
        return struct.pack("<I", int(last) | (2 << 1) | (size << 3))[:3] + body


def xxh64(b):
    """XXH64, seed 0 (the published algorithm)"""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, v: (rotl((acc + v * P2) & M, 31) * P1) & M
    n, i = len(b), 0
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, (-P1) & M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(b[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(b[i:i + 8], "little")), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(b[i:i + 4], "little") * P1) & M, 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = (rotl(h ^ (b[i] * P5) & M, 11) * P1) & M
        i += 1
    h ^= h >> 33; h = (h * P2) & M; h ^= h >> 29; h = (h * P3) & M; h ^= h >> 32
    return h


def frame(blocks, *, fcs="auto", single_segment=True, window=None, checksum=False, tags=(), **forge):
    """fcs: bytes of the content size field (0, 1, 2, 4, 8; "auto": the smallest that holds the size).  window: the window descriptor
    byte of a frame that is not single-segment (default: the smallest window that holds the content).
    forge: fcs_value (the size written), reserved=1, dict_id=1..3, cut=n (bytes kept), sum_xor (damage to the checksum)"""
    B = _Builder()
    body, tree_age = b"", 0
    for i, blk in enumerate(blocks):
        if blk["kind"] == "comp" and blk["lits"]["kind"] == "huf":
            tree_age = 0
        tree_age += 1
        body += B.block(blk, i == len(blocks) - 1, tree_age)
    if sum(1 for blk in blocks if blk["kind"] == "comp") >= 2 and any(blk["kind"] != "comp" for blk in blocks[1:-1]):
        B.tags.add("mixed_blocks")
    n = len(B.out)
    if fcs == "auto":
        fcs = 1 if n < 256 else 2 if n < 65536 + 256 else 4
    if not single_segment and fcs == 1:
        fcs = 2 if n >= 256 else 4
    if single_segment:
        assert fcs in (1, 2, 4, 8)
    val = forge.get("fcs_value", n)
    if fcs == 2:
        assert val >= 256
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    fhd = (flag << 6) | (int(single_segment) << 5) | (forge.get("reserved", 0) << 3) | (int(checksum) << 2) | forge.get("dict_id", 0)
    head = MAGIC + bytes([fhd])
    if not single_segment:
        if window is None:
            e = 0
            while (1 << (10 + e)) < n:
                e += 1
            window = e << 3
        head += bytes([window])
        if (window >> 3) + 10 > 31:
            B.ok = False
        B.tags.add("window_fcs" if fcs else "window_nofcs")
    else:
        B.tags.add("fcs%d" % fcs)
    if fcs:
        head += (val - 256 if fcs == 2 else val).to_bytes(fcs, "little")
    data = head + body
    if checksum:
        data += struct.pack("<I", (xxh64(bytes(B.out)) & 0xFFFFFFFF) ^ forge.get("sum_xor", 0))
        B.tags.add("checksum")
    if set(forge) & {"fcs_value", "reserved", "dict_id", "cut", "sum_xor"}:
        B.ok = False
    if "cut" in forge:
        data = data[:forge["cut"]]
    if B.ok:
        SPECS[data] = list(blocks)
    return Crafted(data, bytes(B.out) if B.ok else None, frozenset(B.tags | set(tags)) if B.ok else frozenset())


SPECS = {}                       # frame bytes -> the block specs frame() was given (valid frames only): what parse_frame is held to


def walk(data):
    """what a test may want to know about a (possibly damaged) frame without decoding it: the frame header descriptor, the declared content
    size (None: none), the largest Block_Size of a block header and, for every compressed block whose literals header can be followed, (bytes of the sequence count with its value,
    the symbol compression modes byte or None).  Stops quietly where the frame stops making sense."""
    info = {"fhd": None, "fcs": None, "blocks": [], "largest_block": 0}
    if len(data) < 5 or data[:4] != MAGIC:
        return info
    fhd = data[4]
    info["fhd"] = fhd
    single, flag = (fhd >> 5) & 1, fhd >> 6
    p = 5 + (0 if single else 1)
    nb = {0: single, 1: 2, 2: 4, 3: 8}[flag]
    if p + nb > len(data):
        return info
    if nb:
        info["fcs"] = int.from_bytes(data[p:p + nb], "little") + (256 if nb == 2 else 0)
    p += nb
    while p + 3 <= len(data):
        bh = int.from_bytes(data[p:p + 3], "little")
        p += 3
        typ, size = (bh >> 1) & 3, bh >> 3
        if typ == 3:
            break
        info["largest_block"] = max(info["largest_block"], size)
        if typ == 2 and p + size <= len(data):
            b = data[p:p + size]
            if b:
                lt, sf = b[0] & 3, (b[0] >> 2) & 3
                v = int.from_bytes(b[:5], "little")
                if lt < 2:
                    hl = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                    ls = v >> 3 & 31 if sf in (0, 2) else v >> 4 & 0xFFF if sf == 1 else v >> 4 & 0xFFFFF
                    q = hl + (ls if lt == 0 else 1)
                else:
                    bits, hl = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
                    q = hl + ((v >> (4 + bits)) & ((1 << bits) - 1))
                if q < len(b):
                    n0 = b[q]
                    k = 1 if n0 < 128 else 3 if n0 == 255 else 2
                    if q + k <= len(b):
                        nseq = n0 if k == 1 else ((n0 - 128) << 8) + b[q + 1] if k == 2 else b[q + 1] + (b[q + 2] << 8) + 0x7F00
                        info["blocks"].append((k, nseq, b[q + k] if q + k < len(b) else None))
        p += size if typ != 1 else 1
        if bh & 1:
            break
    return info


# ---- the catalogue ----
ROUTES = tuple(
    "fcs1 fcs2 fcs4 fcs8 window_nofcs window_fcs checksum "
    "raw_0 raw_1 raw_63 raw_64 raw_65 raw_131072 rle_0 rle_1 rle_63 rle_64 rle_65 rle_131072 raw_last_empty rle_last_empty comp_last_empty "
    "mixed_blocks "
    "lit_raw_sf0 lit_raw_sf1 lit_raw_sf2 lit_raw_sf3 lit_rle_sf0 lit_rle_sf1 lit_rle_sf2 lit_rle_sf3 lit_huf_sf0 lit_huf_sf1 lit_huf_sf2 lit_huf_sf3 "
    "lit_rle_sequences huf_1stream huf_4stream_6 huf_4stream_7 huf_4stream_511 huf_4stream_512 huf_two_tile "
    "weights_direct_odd weights_direct_even weights_fse huf_maxlen_11 treeless_prev treeless_across_raw lit_leftover lit_none "
    "nseq_0 nseq_1 nseq_63 nseq_64 nseq_65 nseq_127 nseq_128 nseq_129 nseq_3byte "
    "ll_predef ll_rle ll_fse of_predef of_rle of_fse ml_predef ml_rle ml_fse "
    "ll_repeat_after_predef ll_repeat_after_rle ll_repeat_after_fse of_repeat_after_predef of_repeat_after_rle of_repeat_after_fse "
    "ml_repeat_after_predef ml_repeat_after_rle ml_repeat_after_fse ll_fse_maxlog of_fse_maxlog ml_fse_maxlog "
    "rep1_llpos rep1_ll0 rep2_llpos rep2_ll0 rep3_llpos rep3_ll0 rep_across_blocks "
    "match_pos1 match_of1_lengths match_periodic match_of_eq_len match_waiting match_straddle_batch match_prev_block "
    "match_long_small_of match_long_big_of ll_code_35_ml_code_52 of_code_20 of_code_21 of_code_22".split())


STRICTER = "stricter_than_libzstd"


def pat(n, seed=1):
    """n bytes that do not repeat soon"""
    out, x = bytearray(n), (seed * 2654435761 + 12345) & 0xFFFFFFFF
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    return bytes(out)


def skew(n, k, seed=1):
    """n bytes over k symbols, the first ones much more frequent (worth a Huffman code)"""
    return bytes(min(k - 1, (8 - (x & 255).bit_length()) * k // 9 + (x >> 8) % 2) for x in struct.unpack("<%dH" % n, pat(2 * n, seed)))


def _catalogue():
    cat = []

    def ok(name, fr, *tags):
        assert fr.expected is not None, name
        cat.append((name, fr.data, fr.expected, frozenset(fr.tags | set(tags))))

    def bad(name, fr):
        cat.append((name, fr.data, None, frozenset()))

    def strict(name, fr):
        """refused by the format and by this project's decoders; libzstd 1.4.8 lets it pass (docs/codecs.md, differences from libzstd)"""
        cat.append((name, fr.data, None, frozenset([STRICTER])))

    P = pat(300)
    # frame header
    ok("fcs 1 byte", frame([raw(P[:9])], fcs=1))
    ok("fcs 2 bytes", frame([raw(P)], fcs=2))
    ok("fcs 4 bytes", frame([raw(P[:9])], fcs=4))
    ok("fcs 8 bytes", frame([raw(P[:9])], fcs=8))
    ok("window, no fcs", frame([raw(P)], single_segment=False, fcs=0))
    ok("window and fcs", frame([raw(P)], single_segment=False, fcs=4))
    ok("checksum", frame([raw(P), comp(lraw(P[:40]), [(3, 9, 5), (30, 4, 1)])], checksum=True))
    bad("checksum wrong", frame([raw(P)], checksum=True, sum_xor=0x100))
    bad("reserved bit", frame([raw(P[:9])], reserved=1))
    bad("window log 32", frame([raw(P)], single_segment=False, fcs=0, window=0xB0))
    bad("window log 41", frame([raw(P)], single_segment=False, fcs=0, window=0xF8))
    bad("header cut in the magic", frame([raw(P)], cut=3))
    bad("header cut before the fcs", frame([raw(P)], fcs=4, cut=7))
    bad("header cut before the window", frame([raw(P)], single_segment=False, fcs=0, cut=5))
    bad("fcs too big", frame([raw(P)], fcs_value=301))
    bad("fcs too small", frame([raw(P)], fcs_value=299))
    two = frame([raw(P[:9])]).data
    strict("two frames back to back", Crafted(two + two, None, frozenset()))
    strict("skippable frame in front", Crafted(b"\x50\x2a\x4d\x18\x03\x00\x00\x00abc" + two, None, frozenset()))
    strict("skippable frame alone", Crafted(b"\x50\x2a\x4d\x18\x03\x00\x00\x00abc", None, frozenset()))
    strict("dictionary id", frame([raw(P[:9])], dict_id=1)._replace(data=frame([raw(P[:9])]).data[:4] + b"\x21\x07\x09" + frame([raw(P[:9])]).data[6:]))
    # blocks
    for n in (0, 1, 63, 64, 65, 131072):
        ok("raw block of %d" % n, frame([raw(pat(n, n))]))
        ok("rle block of %d" % n, frame([rle(n & 255 | 1, n)]))
    ok("empty raw block first", frame([raw(b""), raw(b"x")]))
    ok("empty compressed block last", frame([raw(P[:5]), comp(lraw(b"", sf=1))]))
    bad("reserved block type", frame([forged(3, 4, b"abcd")]))
    strict("raw block of 131073", frame([raw(bytes(131073))]))
    strict("rle block of 131073", frame([rle(7, 131073)]))
    bad("compressed block of 131073", frame([comp(lraw(pat(131070, 5), sf=3))]))
    bad("compressed block of 0", frame([raw(b"abc"), forged(2, 0)]))
    bad("compressed block of 1", frame([raw(b"abc"), forged(2, 1, b"\0")]))
    bad("compressed block of 2", frame([forged(2, 2, b"\0\0")]))
    H = skew(200, 7)
    WH = Huf.for_data(H + bytes(range(7))).weights                                   # one tree for all of H: the treeless blocks below use every symbol of it
    ok("raw + compressed + rle + compressed", frame([
        raw(P[:50]),
        comp(lhuf(H[:100], weights=WH), [(5, 6, 13), (9, 7, 33), (20, 5, 2)], modes=(("fse", 6), ("fse", 6), ("fse", 6)),
             cover={"ll": range(25), "ml": range(40), "of": range(9)}),
        rle(0xAA, 77),
        comp(ltreeless(H[100:]), [(4, 8, 1), (7, 30, 2), (0, 3, 3), (11, 9, 170)], modes=("repeat", "repeat", "repeat"))]))
    # literals
    for sf, n in ((0, 30), (1, 300), (2, 31), (3, 300)):
        ok("raw literals, size format %d" % sf, frame([comp(lraw(pat(n, sf), sf=sf))]))
        ok("rle literals, size format %d" % sf, frame([comp(lrle(0x41 + sf, n, sf=sf))]))
    ok("raw literals of 5000, 20-bit size", frame([comp(lraw(pat(5000, 3)))]))
    ok("rle literals of 70000", frame([comp(lrle(9, 70000))]))
    ok("rle literals cut by sequences", frame([raw(P[:40]), comp(lrle(0x55, 300), [(0, 4, 9), (17, 5, 1), (200, 140, 33), (16, 3, 2), (40, 3, 4)])]), "lit_rle_sequences")
    ok("huffman, 1 stream", frame([comp(lhuf(skew(100, 5)))]))
    ok("huffman, 1 stream of 1000 literals", frame([comp(lhuf(skew(1000, 40, 2), desc="fse"))]))
    for n in (6, 7, 511, 512):
        ok("huffman, 4 streams of %d" % n, frame([comp(lhuf(skew(n, 6, n), streams=4))]))
    ok("huffman, 4 streams, sequences before 512", frame([comp(lhuf(skew(511, 9, 3), streams=4), [(100, 20, 53), (0, 200, 4), (300, 3, 1)])]))
    ok("huffman, 4 streams, sequences from 512", frame([comp(lhuf(skew(513, 9, 4), streams=4), [(100, 20, 53), (0, 200, 4), (300, 3, 1)])]))
    ok("huffman, 4 streams of 9000", frame([comp(lhuf(skew(9000, 30, 5), streams=4, desc="fse"), [(4000, 1000, 3003), (4999, 5, 2)])]))
    ok("huffman, 4 streams of 70000", frame([comp(lhuf(skew(70000, 200, 6), streams=4, desc="fse"))]))
    ok("huffman, 4 streams, 14-bit sizes on a small section", frame([comp(lhuf(skew(600, 6, 8), streams=4, sf=2))]))
    ok("weights direct, odd count", frame([comp(lhuf(bytes([0, 1, 2, 3] * 9 + [0] * 30)))]))            # 3 weights listed
    ok("weights direct, even count", frame([comp(lhuf(bytes([0, 1, 2, 3, 4] * 9 + [0] * 30)))]))        # 4 weights listed
    ok("weights direct, 128 listed", frame([comp(lhuf(bytes(range(129)) * 2 + bytes(60)))]))
    ok("weights fse, 255 listed", frame([comp(lhuf(bytes(range(256)) * 2 + bytes(300) + bytes([7]) * 100, desc="fse", streams=4))]))
    W11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]
    D11 = bytes([0] * 40 + [1] * 20 + list(range(12)) * 3)
    ok("longest code 11, direct", frame([comp(lhuf(D11, weights=W11))]))
    ok("longest code 11, fse, 4 streams", frame([comp(lhuf(D11 * 6, weights=W11, desc="fse", streams=4))]))
    bad("weights do not fill a power of two", frame([comp(lhuf(bytes([0, 1, 2] * 5), weights=[3, 1, 1]))]))
    bad("longest code 12", frame([comp(lhuf(D11 + b"\x0c", weights=[12] + W11))]))
    bad("huffman stream ends in a zero byte", frame([comp(lhuf(skew(100, 5), stream=lambda s: s[:-1] + b"\0"))]))
    bad("huffman stream one byte short", frame([comp(lhuf(skew(100, 5), stream=lambda s: s[1:]))]))
    bad("huffman stream one byte long", frame([comp(lhuf(skew(100, 5), stream=lambda s: b"\0" + s))]))
    bad("4 huffman streams, one ends in a zero byte", frame([comp(lhuf(skew(600, 5), streams=4, stream=lambda s: s[:-1] + b"\0"))]))
    ok("treeless after the previous block", frame([comp(lhuf(H[:90], weights=WH)), comp(ltreeless(H[90:]))]))
    ok("treeless, 4 streams of 600", frame([comp(lhuf(skew(50, 7, 2), weights=WH)), comp(ltreeless(skew(600, 7, 3), streams=4), [(10, 40, 23)])]))
    ok("treeless across a raw block", frame([comp(lhuf(H[:90], weights=WH)), raw(b"between"), comp(lraw(b"no tree here")), comp(ltreeless(H[90:]))]))
    bad("treeless first", frame([raw(P[:20]), comp(ltreeless(H[:90]))]))
    ok("literals left over", frame([comp(lraw(P[:60]), [(10, 5, 7)])]))
    ok("huffman literals left over", frame([comp(lhuf(H), [(10, 5, 7), (50, 70, 1)])]))
    ok("no literals at all", frame([raw(P[:40]), comp(lraw(b""), [(0, 10, 13), (0, 5, 33)])]))
    # sequence count
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 0x7F00):
        ok("%d sequences" % n, frame([comp(lraw(pat(n + 2, n)), [(1, 3, 4)] * min(n, 1) + [(1, 3, 1)] * (n - 1))]))
    ok("5 sequences, count in two bytes", frame([comp(lraw(P[:9]), [(1, 3, 4)] + [(1, 3, 1)] * 4, nseq_bytes=2)]))
    ok("300 sequences over huffman literals", frame([comp(lhuf(skew(700, 12, 9), streams=4), [(2, 4, 5)] + [(2, 3 + k % 7, 1 + k % 3) for k in range(299)])]))
    bad("0 sequences and a byte behind", frame([comp(lraw(P[:9]), tail=b"\0")]))
    bad("0 sequences in two bytes", frame([comp(lraw(P[:9]), nseq_bytes=2)]))
    strict("0 sequences in two bytes and a modes byte", frame([comp(lraw(P[:9]), nseq_bytes=2, tail=b"\0")]))
    # table modes
    PRE = raw(pat(1100, 99))                                       # history for the offsets below
    S3 = [(2, 5, 7)] * 3
    SV = [(2, 5, 7), (0, 3, 1), (17, 40, 60), (1, 4, 9), (3, 130, 2), (25, 7, 1000), (2, 5, 7)]
    for m in ("predef", "rle", "fse"):
        seqs = S3 if m == "rle" else SV
        ok("all tables %s, then repeated" % m, frame([PRE, comp(lraw(pat(60, 2)), seqs, modes=(m, m, m)),
                                                      comp(lraw(pat(60, 3)), list(reversed(seqs)), modes=("repeat", "repeat", "repeat"))]))
    ok("mixed modes", frame([PRE, comp(lraw(pat(60, 2)), [(2, 5, 60), (2, 9, 7), (2, 3, 1)], modes=("rle", "fse", "predef")),
                             comp(lraw(pat(60, 3)), [(2, 5, 7), (7, 5, 60), (9, 5, 1)], modes=("predef", "repeat", "rle")),
                             comp(lraw(pat(60, 4)), [(2, 5, 7), (7, 5, 2), (9, 5, 1)], modes=("fse", "predef", "repeat"))]))
    bad("repeat with no table", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=("repeat", "predef", "predef"))]))
    bad("repeat offsets table with no table", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=("predef", "repeat", "predef"))]))
    bad("repeat match table with no table", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=("predef", "predef", "repeat"))]))
    for which, sym in (("ll", 36), ("of", 32), ("ml", 53)):
        bad("rle %s symbol %d" % (which, sym), frame([PRE, comp(lraw(pat(60, 2)), S3, modes=("rle", "rle", "rle"), rle_sym={which: sym})]))
    ok("fse tables at the largest logs", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=(("fse", 9), ("fse", 8), ("fse", 9)))]))
    ok("fse tables with less-than-one counts", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=(
        ("fse", 6, [30, 10, 12, 8] + [0] * 12 + [-1, 0, 0, 0, 3]), ("fse", 5, [-1, 8, 10, 6, 0, 4, 0, 0, 0, 3]), "predef"))]))
    bad("fse ll table log 10", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=(("fse", 10), "predef", "predef"))]))
    bad("fse of table log 9", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=("predef", ("fse", 9), "predef"))]))
    bad("fse ml table log 10", frame([PRE, comp(lraw(pat(60, 2)), SV, modes=("predef", "predef", ("fse", 10)))]))
    strict("modes byte with reserved bits", frame([PRE, comp(lraw(pat(60, 2)), SV, modes_low=1)]))
    # repeat offsets
    R = [(8, 3, 8), (2, 3, 10), (3, 4, 12), (1, 3, 1), (1, 3, 2), (1, 3, 3), (0, 3, 1), (0, 3, 2), (0, 3, 3), (2, 3, 3), (0, 4, 3)]
    ok("every repeat code", frame([comp(lraw(pat(30, 6)), R)]))
    ok("repeat codes from the start values", frame([raw(P[:20]), comp(lraw(pat(9, 6)), [(1, 3, 3), (1, 3, 2), (0, 3, 1), (0, 5, 3)])]))
    bad("rep0 - 1 = 0", frame([comp(lraw(pat(9, 6)), [(2, 3, 4), (0, 3, 3)])]))
    ok("history from block to block", frame([comp(lraw(pat(30, 6)), R), comp(lraw(pat(9, 7)), [(1, 6, 1), (0, 3, 1), (2, 5, 3)]),
                                             comp(lraw(pat(9, 8)), [(0, 9, 3), (3, 3, 2)])]))
    # matches
    ok("match of 3 at offset 1 at position 1", frame([comp(lraw(b"Q"), [(1, 3, 4)])]), "match_pos1")
    ok("offset 1, lengths 3 4 5 128 129", frame([comp(lraw(b"abcde"), [(1, 3, 4), (1, 4, 1), (1, 5, 1), (1, 128, 1), (1, 129, 1)])]), "match_of1_lengths")
    ok("offsets 2 and 3, long", frame([comp(lraw(b"abcde"), [(2, 100, 5), (3, 200, 6), (0, 129, 5), (0, 1000, 6)])]), "match_periodic")
    ok("offset = length and length - 1", frame([raw(P[:200]), comp(lraw(pat(40, 9)), [(10, 10, 13), (10, 11, 13), (10, 140, 143), (10, 141, 143)])]), "match_of_eq_len")
    ok("matches that wait on matches", frame([comp(lraw(pat(6, 9)), [(4, 4, 7), (1, 4, 7), (1, 12, 15), (0, 20, 22), (0, 200, 43), (0, 7, 9)])]), "match_waiting")
    ok("source across the batch's first byte", frame([raw(P[:10]), comp(lraw(pat(140, 10)), [(2, 3 + k % 5, 4 + k % 9) for k in range(64)] + [(2, 8, 7), (2, 150, 9)])]),
       "match_straddle_batch")
    ok("source in the previous block", frame([raw(P[:30]), comp(lraw(pat(9, 11)), [(1, 10, 8), (0, 25, 33), (3, 200, 53)]), rle(5, 9),
                                              comp(lraw(pat(3, 12)), [(0, 12, 15), (1, 300, 250)])]), "match_prev_block")
    ok("match over 128, offset below length", frame([comp(lraw(pat(200, 13)), [(200, 150, 10), (0, 1000, 140)])]), "match_long_small_of")
    ok("match over 128, offset at least length", frame([comp(lraw(pat(400, 13)), [(200, 150, 183), (200, 129, 132), (0, 300, 403)])]), "match_long_big_of")
    bad("offset one past the output", frame([comp(lraw(pat(9, 14)), [(5, 3, 9)])]))
    bad("offset one past the output in a later block", frame([raw(P[:20]), comp(lraw(pat(9, 14)), [(5, 3, 4), (2, 3, 34)])]))
    f = frame([comp(lhuf(H[:100]), [(10, 60, 5)])])
    bad("match into huffman literals still to come", f._replace(data=frame([comp(lhuf(H[:100]), [(10, 60, 5)])], fcs_value=len(f.expected) - 30).data))
    f = frame([comp(lraw(P[:20]), [(20, 60, 5)])])
    bad("match past the content size", f._replace(data=frame([comp(lraw(P[:20]), [(20, 60, 5)])], fcs_value=len(f.expected) - 1).data))
    bad("literals run out", frame([comp(lraw(P[:20]), [(10, 3, 5), (11, 3, 1)])]))
    # length and offset codes
    ok("largest length codes in one sequence", frame([comp(lraw(pat(65541, 15)), [(65541, 65546, 1003)])]))
    ok("every length code", frame([raw(P[:60]), comp(lraw(pat(3000, 16)), [(LL_BASE[c % 30] + (c % 3 if LL_BITS[c % 30] else 0), ML_BASE[c] + (1 if ML_BITS[c] else 0), 4 + c)
                                                               for c in range(46)])]))
    for code, nblk in ((20, 9), (21, 17), (22, 33)):
        total = nblk * 131072
        ofv = total + 4 - 131069 + 3
        assert ofv.bit_length() - 1 == code
        ok("offset code %d" % code, frame([raw(pat(131072, code))] + [rle(k, 131072) for k in range(1, nblk)] + [comp(lraw(b"wxyz"), [(4, 8, ofv), (0, 300, 1)])]))
    # bit stream
    strict("sequence stream with bits left over", frame([PRE, comp(lraw(pat(60, 2)), SV, spare_bits=3)]))
    strict("sequence stream with a byte left over", frame([PRE, comp(lraw(pat(60, 2)), SV, spare_bits=8)]))
    bad("sequence stream overrun", frame([PRE, comp(lraw(pat(60, 2)), SV, stream=lambda s: s[1:])]))
    bad("sequence stream ends in a zero byte", frame([PRE, comp(lraw(pat(60, 2)), SV, stream=lambda s: s + b"\0")]))
    return cat


CATALOGUE = _catalogue()


# ================================================================ reading frames (for the ENCODER's tests: tests/test_zstd_encode_craft.py)
# parse_frame follows RFC 8878 section by section and keeps what it read: a test asks it WHICH block, literals form, description,
# stream sizes and sequences a frame holds, not only what bytes come out.
class BackReader:
    """a stream read from its last bit down (RFC 8878 4.1): the highest set bit of the last byte is the end mark; take() never reads in
    front of the first byte, take_padded() reads zeros there (how the end of an FSE stream of weights is found)"""
    def __init__(self, b):
        if not len(b) or b[-1] == 0:
            raise ValueError("bit stream without an end mark")
        self.b = bytes(b)
        self.n = 8 * (len(b) - 1) + b[-1].bit_length() - 1           # bits still to read: bit n - 1 is the next one

    def take(self, nb):
        if nb > self.n:
            raise ValueError("bit stream overrun")
        hi = self.n
        self.n = lo = hi - nb
        return (int.from_bytes(self.b[lo >> 3:(hi + 7) >> 3], "little") >> (lo & 7)) & ((1 << nb) - 1)


def read_ncount(b, max_log, max_sym):
    """the count header of an FSE table (RFC 8878 4.1.1; the reader of ncount()) -> (norm, log, bytes read)"""
    v, avail, pos = int.from_bytes(b, "little"), 8 * len(b), 4
    if avail < 4:
        raise ValueError("count header cut")
    log = (v & 15) + 5
    if log > max_log:
        raise ValueError("accuracy log %d above %d" % (log, max_log))
    remaining, threshold, nb, norm, prev0 = (1 << log) + 1, 1 << log, log + 1, [], False
    while remaining > 1:
        if prev0:
            while True:
                if pos + 2 > avail:
                    raise ValueError("count header cut")
                r = (v >> pos) & 3
                pos += 2
                norm += [0] * r
                if r != 3:
                    break
        if len(norm) > max_sym:
            raise ValueError("more symbols than the alphabet holds")
        if pos + nb > avail + 7:                             # (a value's unread upper bits may lie in the padding of the last byte)
            raise ValueError("count header cut")
        maxv = 2 * threshold - 1 - remaining
        val = (v >> pos) & (threshold - 1)
        if val < maxv:
            pos += nb - 1
        else:
            val = (v >> pos) & (2 * threshold - 1)
            pos += nb
            if val >= threshold:
                val -= maxv
        if pos > avail:
            raise ValueError("count header cut")
        c = val - 1
        remaining -= abs(c)
        if remaining < 1:
            raise ValueError("counts exceed the table")
        norm.append(c)
        prev0 = c == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    return norm, log, (pos + 7) // 8


def read_tree(b):
    """a Huffman tree description at the head of b (RFC 8878 4.2.1) -> (Huf, form, bytes, the FSE stream ended exactly)"""
    if not len(b):
        raise ValueError("no tree description")
    hb, exact = b[0], True
    if hb >= 128:
        n = hb - 127
        size = 1 + (n + 1) // 2
        if size > len(b):
            raise ValueError("tree description cut")
        w = [(b[1 + k // 2] >> (0 if k & 1 else 4)) & 15 for k in range(n)]
        form = "direct"
    else:
        size = 1 + hb
        if hb < 2 or size > len(b):
            raise ValueError("tree description cut")
        norm, log, used = read_ncount(b[1:size], 6, 12)
        t = Fse(norm, log)
        r = BackReader(b[1 + used:size])
        st, w, k = [r.take(log), r.take(log)], [], 0
        while True:                                          # two states in turn; the stream is over when a state's bits are not all there
            w.append(t.sym[st[k]])
            if t.nb[st[k]] > r.n:
                w.append(t.sym[st[k ^ 1]])
                break
            st[k] = t.base[st[k]] + r.take(t.nb[st[k]])
            k ^= 1
            if len(w) > 255:
                raise ValueError("more than 255 weights")
        exact = r.n == 0
        form = "fse"
    if len(w) > 255:
        raise ValueError("more than 255 weights")
    total = sum(1 << (x - 1) for x in w if x)
    if total == 0 or max(w) > 11:
        raise ValueError("weights of no tree")
    rest = (1 << total.bit_length()) - total
    if rest & (rest - 1) or total.bit_length() > 11:
        raise ValueError("weights do not complete to a power of two of at most 11 bits")
    return Huf(w + [rest.bit_length()]), form, size, exact


def _huf_table(huf):
    """decode table over maxbits bits: symbol | length << 8"""
    mb = huf.maxbits
    tab = [0] * (1 << mb)
    for s, (c, nb) in huf.code.items():
        lo = c << (mb - nb)
        tab[lo:lo + (1 << (mb - nb))] = [s | (nb << 8)] * (1 << (mb - nb))
    return tab


def _huf_stream(tab, mb, b, count):
    """count symbols from one Huffman stream, which must end exactly at its first bit"""
    n = BackReader(b).n
    mask, out, at = (1 << mb) - 1, bytearray(count), (n + 7) >> 3
    acc, na = 0, 0                                                   # the next na bits of the stream, the first one on top
    for i in range(count):
        if na < mb and at:
            lo = max(0, at - 8)
            k = min(n, 8 * at) - 8 * lo                              # (the first refill leaves the end mark out)
            acc = (acc << k) | (int.from_bytes(b[lo:at], "little") & ((1 << k) - 1))
            na, at = na + k, lo
        e = tab[(acc >> (na - mb)) & mask] if na >= mb else tab[(acc << (mb - na)) & mask]
        na -= e >> 8
        if na < 0:
            raise ValueError("Huffman stream overrun")
        acc &= (1 << na) - 1
        out[i] = e & 255
    if na or at:
        raise ValueError("Huffman stream does not end on its first bit")
    return bytes(out)


def _read_literals(b, prev_huf):
    """the literals section at the head of block content b -> (namespace, literals, bytes, the tree in force)"""
    if not len(b):
        raise ValueError("no literals section")
    kind, sf = ("raw", "rle", "huf", "treeless")[b[0] & 3], (b[0] >> 2) & 3
    v = int.from_bytes(b[:5], "little")
    L = types.SimpleNamespace(kind=kind, sf=sf, csize=None, streams=0, stream_sizes=(), desc=None, desc_len=0, desc_exact=True, weights=None, lengths=None)
    if kind in ("raw", "rle"):
        L.hl = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        L.regen = v >> 3 & 31 if L.hl == 1 else v >> 4 & 0xFFF if L.hl == 2 else v >> 4 & 0xFFFFF
        need = L.hl + (L.regen if kind == "raw" else 1)
        if need > len(b) or L.regen > 131072:
            raise ValueError("literals section cut")
        return L, (b[L.hl:need] if kind == "raw" else b[L.hl:L.hl + 1] * L.regen), need, prev_huf
    bits, L.hl = {0: (10, 3), 1: (10, 3), 2: (14, 4), 3: (18, 5)}[sf]
    L.regen, L.csize, L.streams = (v >> 4) & ((1 << bits) - 1), (v >> (4 + bits)) & ((1 << bits) - 1), 1 if sf == 0 else 4
    if L.hl + L.csize > len(b) or L.regen > 131072:
        raise ValueError("literals section cut")
    body = b[L.hl:L.hl + L.csize]
    if kind == "huf":
        huf, L.desc, L.desc_len, L.desc_exact = read_tree(body)
        body = body[L.desc_len:]
    else:
        if prev_huf is None:
            raise ValueError("treeless literals with no tree")
        huf = prev_huf
    L.weights = list(huf.weights)
    L.lengths = [huf.maxbits + 1 - w if w else 0 for w in huf.weights]
    tab = _huf_table(huf)
    if L.streams == 1:
        L.stream_sizes = (len(body),)
        lits = _huf_stream(tab, huf.maxbits, body, L.regen)
    else:
        if len(body) < 6:
            raise ValueError("no jump table")
        s = struct.unpack("<3H", body[:6])
        s += (len(body) - 6 - sum(s),)
        if s[3] < 0:
            raise ValueError("jump table beyond the section")
        L.stream_sizes = s
        per, at, parts = (L.regen + 3) // 4, 6, []
        if 3 * per > L.regen:
            raise ValueError("four streams for %d literals" % L.regen)
        for k in range(4):
            parts.append(_huf_stream(tab, huf.maxbits, body[at:at + s[k]], per if k < 3 else L.regen - 3 * per))
            at += s[k]
        lits = b"".join(parts)
    return L, lits, L.hl + L.csize, huf


def parse_frame(data):
    """One frame, read as RFC 8878 says, with everything kept: a namespace of
      fhd, single_segment, window_log, fcs (None: no content size field), fcs_bytes, checksum (the stored one, or None)
      blocks     one namespace per block: type (0 raw, 1 RLE, 2 compressed), size (Block_Size), last, data (what the block regenerates) and,
                 for a compressed block, lit (kind raw | rle | huf | treeless, sf, hl header bytes, regen, csize, streams, stream_sizes as the
                 jump table says, desc direct | fse, desc_len, desc_exact, weights, lengths), literals, nseq, nseq_bytes, modes (the byte, None
                 without sequences), rle_codes {"ll" | "of" | "ml": code} of the tables in RLE mode, seqs [(literal length, match length,
                 Offset_Value)], states (the three last states, LL OF ML)
      content    the blocks' data in a row
      trailing   what follows the frame
    ValueError for anything the format forbids: reserved bits and types, a window beyond 2^31, sizes that do not add up, code lengths above
    11 bits, weights that complete no tree, streams that do not end exactly where they must, tables that are not there, offsets beyond the output,
    a content size or checksum that is not the content's.  (A dictionary id is refused too: no dictionary is at hand.)"""
    data = bytes(data)
    if len(data) < 5 or data[:4] != MAGIC:
        raise ValueError("no frame")
    fhd = data[4]
    single, flag = (fhd >> 5) & 1, fhd >> 6
    if fhd & 0x08:
        raise ValueError("reserved bit")
    if fhd & 3:
        raise ValueError("dictionary id")
    F = types.SimpleNamespace(fhd=fhd, single_segment=bool(single), window_log=None, fcs=None, blocks=[], checksum=None)
    p = 5
    if not single:
        if p >= len(data):
            raise ValueError("header cut")
        F.window_log = 10 + (data[p] >> 3)
        if F.window_log > 31:
            raise ValueError("window log %d" % F.window_log)
        p += 1
    F.fcs_bytes = {0: single, 1: 2, 2: 4, 3: 8}[flag]
    if p + F.fcs_bytes > len(data):
        raise ValueError("header cut")
    if F.fcs_bytes:
        F.fcs = int.from_bytes(data[p:p + F.fcs_bytes], "little") + (256 if F.fcs_bytes == 2 else 0)
    p += F.fcs_bytes
    out, rep, huf, tabs = bytearray(), [1, 4, 8], None, {"ll": None, "of": None, "ml": None}
    while True:
        if p + 3 > len(data):
            raise ValueError("block header cut")
        bh = int.from_bytes(data[p:p + 3], "little")
        p += 3
        B = types.SimpleNamespace(type=(bh >> 1) & 3, size=bh >> 3, last=bool(bh & 1), lit=None, literals=None, nseq=0, nseq_bytes=0, modes=None,
                                  rle_codes={}, seqs=[], states=None)
        if B.type == 3 or B.size > 131072:
            raise ValueError("block type %d, size %d" % (B.type, B.size))
        start = len(out)
        if B.type == 0:
            if p + B.size > len(data):
                raise ValueError("raw block cut")
            out += data[p:p + B.size]
            p += B.size
        elif B.type == 1:
            if p + 1 > len(data):
                raise ValueError("RLE block cut")
            out += data[p:p + 1] * B.size
            p += 1
        else:
            if B.size < 3 or p + B.size > len(data):                   # (literals header + sequence count: libzstd's MIN_CBLOCK_SIZE)
                raise ValueError("compressed block of %d bytes" % B.size)
            b = data[p:p + B.size]
            p += B.size
            B.lit, B.literals, q, huf = _read_literals(b, huf)
            if q >= len(b):
                raise ValueError("no sequences section")
            n0 = b[q]
            B.nseq_bytes = 1 if n0 < 128 else 3 if n0 == 255 else 2
            if q + B.nseq_bytes > len(b):
                raise ValueError("sequence count cut")
            B.nseq = n0 if n0 < 128 else b[q + 1] + (b[q + 2] << 8) + 0x7F00 if n0 == 255 else ((n0 - 128) << 8) + b[q + 1]
            q += B.nseq_bytes
            li = 0
            if B.nseq == 0:
                if B.nseq_bytes > 1 or q != len(b):
                    raise ValueError("no sequences, and bytes behind the count")
            else:
                if q >= len(b):
                    raise ValueError("no modes byte")
                B.modes = b[q]
                q += 1
                if B.modes & 3:
                    raise ValueError("reserved bits in the modes byte")
                for which, shift in (("ll", 6), ("of", 4), ("ml", 2)):
                    m = (B.modes >> shift) & 3
                    if m == 0:
                        tabs[which] = Fse(*DEF[which])
                    elif m == 1:
                        if q >= len(b) or b[q] > MAX_SYM[which]:
                            raise ValueError("RLE table of %s" % which)
                        tabs[which] = Fse.rle(b[q])
                        B.rle_codes[which] = b[q]
                        q += 1
                    elif m == 2:
                        norm, log, used = read_ncount(b[q:], MAX_LOG[which], MAX_SYM[which])
                        tabs[which] = Fse(norm, log)
                        q += used
                    elif tabs[which] is None:
                        raise ValueError("repeat mode with no %s table" % which)
                r = BackReader(b[q:])
                tl, to, tm = tabs["ll"], tabs["of"], tabs["ml"]
                sl, so, sm = r.take(tl.log), r.take(to.log), r.take(tm.log)
                for k in range(B.nseq):
                    ofc, mlc, llc = to.sym[so], tm.sym[sm], tl.sym[sl]
                    ofv = (1 << ofc) + r.take(ofc)
                    ml = ML_BASE[mlc] + r.take(ML_BITS[mlc])
                    ll = LL_BASE[llc] + r.take(LL_BITS[llc])
                    B.seqs.append((ll, ml, ofv))
                    if ofv > 3:
                        off = ofv - 3
                        rep = [off, rep[0], rep[1]]
                    else:
                        idx = ofv - 1 + (ll == 0)
                        if idx == 0:
                            off = rep[0]
                        else:
                            off = rep[idx] if idx < 3 else rep[0] - 1
                            rep = [off, rep[0], rep[1]] if idx > 1 else [off, rep[0], rep[2]]
                    if li + ll > len(B.literals):
                        raise ValueError("literals run out")
                    out += B.literals[li:li + ll]
                    li += ll
                    if off == 0 or off > len(out):
                        raise ValueError("offset %d at %d" % (off, len(out)))
                    if off >= ml:
                        out += out[len(out) - off:len(out) - off + ml]
                    else:
                        out += (bytes(out[-off:]) * (ml // off + 1))[:ml]
                    if k + 1 < B.nseq:
                        sl = tl.base[sl] + r.take(tl.nb[sl])
                        sm = tm.base[sm] + r.take(tm.nb[sm])
                        so = to.base[so] + r.take(to.nb[so])
                if r.n != 0:
                    raise ValueError("%d bits of the sequence stream left over" % r.n)
                B.states = (sl, so, sm)
            out += B.literals[li:]
        B.data = bytes(out[start:])
        F.blocks.append(B)
        if B.last:
            break
    if fhd & 4:
        if p + 4 > len(data):
            raise ValueError("checksum cut")
        (F.checksum,) = struct.unpack_from("<I", data, p)
        p += 4
        if F.checksum != xxh64(bytes(out)) & 0xFFFFFFFF:
            raise ValueError("checksum")
    if F.fcs is not None and F.fcs != len(out):
        raise ValueError("content size %d, content %d" % (F.fcs, len(out)))
    F.content, F.trailing = bytes(out), data[p:]
    return F


# ================================================================ the ENCODER's free choices, restated (csrc/zstd_enc_dev.h)
# One copy of each.  What the encoder MUST do is restated here: where it cuts, which runs are sequences, when it takes them.  Its code
# lengths are its own choice (assign_lengths_wave, build_lengths): the tests state properties of the parsed block for them, not a second encoder.
import functools   # noqa: E402
import re          # noqa: E402

import numpy as np   # noqa: E402

import deflate_craft as dc   # noqa: E402

ZBLOCK = 16384                   # DEFL_BLK: the staged form cuts there; the fused kernels hold at most one block
ZSTD_RMIN = 5                    # a run of at least this many equal bytes is a sequence
ZMAXBITS = 11                    # ZSTD_MAXBITS
STALE_FILL = b"\x00\x00\xe5\x00\x00\x00"    # the GPU tests fill the record slots with its first four bytes, over and over (entry stale_bytes_behind_short_block)


def zenc_pieces(payload):
    """the blocks of a payload: cut at every 16384 bytes; an empty payload is one empty block"""
    return [payload[i:i + ZBLOCK] for i in range(0, len(payload), ZBLOCK)] or [b""]


def zenc_tokens(block):
    """(literals, [(literal length, match length)], taken) of ONE block: a run of R >= 5 equal bytes is its first byte as a literal plus one
    match of R - 1 at offset 1; `taken` is the `use` expression of zstd_tokenise, verbatim, and False for blocks under 64 bytes.  (When it is
    False the block's literals are the block itself.)"""
    lits, seqs, pend = bytearray(), [], 0
    for s, r in dc.runs_of(block):
        if r >= ZSTD_RMIN:
            lits.append(block[s])
            seqs.append((pend + 1, r - 1))
            pend = 0
        else:
            lits += block[s:s + r]
            pend += r
    blen, nlit, nseq = len(block), len(lits), len(seqs)
    use = (nseq != 0 and not (nseq == 1 and nlit == 1) and nlit + 4 * nseq + 8 <= blen and
           3 + nlit + 4 + ((12 * nseq + (nlit >> 2) + ((blen - nlit) >> 3) + 20) >> 3) + 1 < blen)
    return bytes(lits), seqs, blen >= 64 and use


def zenc_literals(block):
    """the literals the block's literals section holds (if it is a compressed block), and its sequences"""
    lits, seqs, taken = zenc_tokens(block)
    return (lits, seqs) if taken else (bytes(block), [])


def zenc_chunk(blen):
    """K of zstd_tokenise: lane t of 256 owns bytes [t K, t K + K)"""
    return ((blen + 255) // 256 + 3) & ~3


def zenc_split(hdr_len, n_samples, plen):
    """literals-only mode (option zstd_sequences = 0), fused kernel, svb-zd: the block lengths of a record — the head (raw), the key bytes,
    then whole blocks — or None where the kernel's rule leaves the record in one piece"""
    at = hdr_len + 12 + ((n_samples + 3) >> 2)
    if at >= 256 and at + 256 <= plen and at <= ZBLOCK:
        return [hdr_len + 12, at - (hdr_len + 12)] + [len(x) for x in zenc_pieces(bytes(plen - at))]
    return None


def ll_code(ll):
    return _code_of(LL_BASE, ll)


def ml_code(ml):
    return _code_of(ML_BASE, ml)


def histogram(data):
    return np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=256).tolist()


def shannon_clamped(freq, limit=ZMAXBITS):
    """min(limit, ceil(log2(N / f))) per symbol in use: where assign_lengths_wave<11> starts"""
    return [min(limit, l) for l in dc.shannon_lengths(freq)]


def kraft(lengths, limit=ZMAXBITS):
    """sum of 2^(limit - l): a code iff <= 2^limit, complete iff equal"""
    return sum(1 << (limit - l) for l in lengths if l)


def limited_lengths(freq, limit=ZMAXBITS):
    """optimal code lengths of at most `limit` bits (package-merge, Larmore and Hirschberg 1990): the test's own yardstick"""
    leaves = sorted((f, (s,)) for s, f in enumerate(freq) if f)
    n = len(leaves)
    assert 2 <= n <= 1 << limit
    cur = list(leaves)
    for _ in range(limit - 1):
        packs = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + packs, key=lambda x: x[0])
    out = [0] * len(freq)
    for _, syms in cur[:2 * n - 2]:
        for s in syms:
            out[s] += 1
    return out


def code_bits(freq, lengths):
    return sum(f * l for f, l in zip(freq, lengths))


def spread(counts):
    """bytes with counts[s] occurrences of symbol s (a dict), no two neighbours equal (the most frequent at most every other byte)"""
    order = [s for s, c in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])) for _ in range(c)]
    n = len(order)
    assert 2 * max(counts.values()) <= n + 1
    out = bytearray(n)
    out[0::2] = bytes(order[:(n + 1) // 2])
    out[1::2] = bytes(order[(n + 1) // 2:])
    assert all(r == 1 for _, r in dc.runs_of(out))
    return bytes(out)


def low4(rng, n, alphabet=bytes(range(4))):
    """n bytes over four small values, no run of four: a Huffman block whose tree description is three bytes"""
    return bytes(dc.background(rng, n, alphabet))


def zenc_payload(e, sig_method=1):
    """the payload of an entry: a solo entry's own bytes, else the oracle's record payload (sig_method 1 svb-zd, 2 ex-zd)"""
    if e["solo"]:
        return e["body"]
    return dc.enc_payload(dict(e, name="zenc:" + e["name"]), sig_method)


ZENC_SIZES = (0, 1, 63, 64, 65, 16383, 16384, 16385, 32768, 32769)
ZENC_KS = ((4, 1001), (32, 7999), (64, 15400))                  # (K, a block length with that K whose last lane chunk is partial)
ZENC_NSEQ = (1, 63, 64, 65, 127, 128, 129, 3275)
ZENC_LL_STEPS = (15, 16, 23, 24, 31, 32, 47, 48, 63, 64, 127, 128, 4097)
ZENC_MB_STEPS = (31, 32, 39, 40, 47, 48, 63, 64, 95, 96, 127, 128, 255, 256, 16379)
ZENC_GEO = ("runs_4_5_6", "run_from_last_byte_of_chunk", "run_from_chunk_offset_k_minus_5", "run_from_chunk_offset_k_minus_4", "run_ends_on_chunk_end",
            "run_over_whole_chunks", "run_across_wave_boundary", "run_spans_a_wave", "run_from_position_0", "run_to_block_end", "partial_last_lane")
ZENC_EDGES = tuple(
    ["size_%d" % n for n in ZENC_SIZES] + ["size_16777221_carry_byte"] +
    ["rle_block", "literal_then_run_two_raw_literals", "run_63_raw", "incompressible_raw", "flat_single_weight_raw",
     "use_first_inequality_refuses", "use_first_inequality_takes", "use_second_inequality_refuses", "use_second_inequality_takes"] +
    ["k%d_%s" % (K, g) for K, _ in ZENC_KS for g in ZENC_GEO] + ["stale_bytes_behind_short_second_block", "stale_bytes_behind_last_lane"] +
    ["nseq_%d" % n for n in ZENC_NSEQ] + ["ll_%d" % n for n in ZENC_LL_STEPS] + ["mb_%d" % n for n in ZENC_MB_STEPS] +
    ["seq_raw_literals_31", "seq_raw_literals_32", "seq_raw_literals_4095", "seq_raw_literals_4096",
     "huf_nl_64", "huf_nl_65", "huf_nl_1023", "huf_nl_1024", "huf_nl_16383", "huf_nl_16384", "huf_csize_near_1023",
     "distinct_2", "distinct_16", "distinct_17", "clamp_oversubscribes", "longest_code_11_exact", "longest_code_11_tree_free",
     "maxsym_127", "maxsym_128", "maxsym_129", "weights_odd", "weights_even", "fse_gap_1", "fse_gap_3", "fse_gap_4", "fse_gap_6",
     "normalise_gives", "normalise_takes"] +
    ["align_phase_%d" % k for k in range(4)] +
    ["lo_head_align_%d" % k for k in range(4)] + ["lo_at_255", "lo_at_256", "lo_tail_255", "lo_tail_256"])


class ZView:
    """what a property is stated on: the payload, its blocks and their restated tokens"""
    def __init__(self, payload):
        self.p = payload
        self.pieces = zenc_pieces(payload)
        self.tok = [zenc_tokens(x) for x in self.pieces]
        self.lits = [zenc_literals(x)[0] for x in self.pieces]
        self.runs = [dc.runs_of(x) for x in self.pieces]

    def hist(self, k=0):
        return histogram(self.lits[k])

    def distinct(self, k=0):
        return sum(1 for f in self.hist(k) if f)

    def maxsym(self, k=0):
        return max(s for s, f in enumerate(self.hist(k)) if f)

    def has_run(self, start, r, k=0):
        return (start, r) in self.runs[k]

    def forced_weights(self, k=0):
        """weights (every symbol up to the last in use) of a block whose literal frequencies are powers of two summing to one: every code no
        larger than the Shannon start has exactly the lengths log2(N / f)"""
        h = self.hist(k)
        N = sum(h)
        assert all(f == 0 or N % f == 0 and (N // f) & (N // f - 1) == 0 for f in h), "not dyadic"
        lens = dc.shannon_lengths(h)
        assert kraft(lens, 15) == 1 << 15
        return [max(lens) + 1 - l if l else 0 for l in lens[:self.maxsym(k) + 1]]


def weight_counts(weights):
    """histogram of the LISTED weights (all but the last symbol's) — what zstd_desc_head normalises"""
    listed = weights[:-1]
    return [listed.count(w) for w in range(max(listed) + 1)]


def normalise_sum(weights):
    """the sum of the first-cut normalised counts of zstd_desc_head (floor(count * 64 / n), at least 1 for a weight in use): below 64 the
    largest count is given the rest, above 64 the largest entries give it back"""
    n = len(weights) - 1
    return sum(max(1, c * 64 // n) for c in weight_counts(weights) if c)


def weight_gaps(weights):
    """lengths of the runs of unused weight values between used ones"""
    used = [w for w, c in enumerate(weight_counts(weights)) if c]
    return [b - a - 1 for a, b in zip(used, used[1:]) if b - a > 1]


@functools.lru_cache(maxsize=None)
def zenc_catalogue():
    """[entry dict]: the smallest payloads that reach each edge of the zstd encoder (csrc/zstd_enc_dev.h).  An entry has name, why, solo
    (True: whole buffers through s5gpu_solo_batch only; False: a record — the oracle's head in front, the crafted bytes as aux bytes, copied
    verbatim — which every route takes), edges (the names of ZENC_EDGES it reaches) and prop, the stated property as a function of a ZView
    of its payload (tests/test_zstd_encode_craft.py asserts it on the CPU for the svb-zd payload).

    Branches of the encoder that no payload reaches, with the argument:
      * RLE literals beside sequences (`lit_mode = distinct == 1 && nl >= 2`): consecutive runs hold different bytes and every run sends its
        first byte as a literal, so literals that are all equal mean that the block is ONE run — nlit = 1, which is not >= 2 (and with
        nseq = 1 the sequence is refused anyway).
      * `3 * per <= nl` false: per = ceil(nl / 4), so 3 per > nl only for nl in {1, 2, 5}; the test sits behind nl >= 64.
      * the 4-byte Huffman header for nl <= 1023 (`csize <= 1023` false while `nl <= 1023`): Huffman literals are kept only if hl + csize
        beats the raw form, 2 + nl beside sequences and nl - 1 without, so a kept csize is below nl.  The clause decides nothing.
      * `at <= DEFL_BLK` of the literals-only split false while the rest holds: the fused kernel holds plen <= 16384 and the rule asks
        at + 256 <= plen.
      * zstd_desc_pack's two "does not fit 127 bytes" returns: no payload found; a description of 255 weights over at most 12 values whose
        counts are tied by the Kraft sum stays below 100 bytes in every block tried."""
    E = []

    def head_of(signal, read_id, fields):
        return dc.enc_payload(dict(name="zenc-head:%r%r%r" % (tuple(signal), read_id, fields), signal=signal, read_id=read_id, fields=fields, aux=b""))

    def solo(name, why, body, edges, prop):
        E.append(dict(name=name, why=why, solo=True, body=bytes(body), edges=tuple(edges), prop=prop))

    def rec(name, why, edges, prop, plen=None, runs=(), aux=None, signal=dc.SIG4, read_id=b"craft0001", fields=dc.FIELDS2, bg=None):
        """plen and runs [(first position, length)] are in PAYLOAD positions: the aux bytes are a background of plen - head bytes (16 letters, no run
        of four) with the runs planted in it, run i of byte RUN_BYTES[i % 16]; or aux as given (bytes, or a function of the head's length)"""
        head = head_of(tuple(signal), read_id, fields)
        if aux is None:
            rng = dc._rng("zenc:" + name)
            pay = bytearray(head) + (dc.background(rng, plen - len(head)) if bg is None else bg(rng, plen - len(head)))
            for i, (s, r) in enumerate(runs):
                assert s >= len(head) and s + r <= plen, (name, s, r)
                pay[s:s + r] = bytes([dc.RUN_BYTES[i % 16]]) * r
            aux = bytes(pay[len(head):])
        elif callable(aux):
            aux = aux(len(head))
        E.append(dict(name=name, why=why, solo=False, signal=tuple(signal), read_id=read_id, fields=fields, aux=bytes(aux), edges=tuple(edges), prop=prop,
                      hdr_len=2 + len(read_id) + 36))

    bgs = lambda name, n: bytes(dc.background(dc._rng("zenc:" + name), n))
    X, Y = b"\xe0", b"\xe1"

    # ---- sizes
    for n in (0, 1, 63, 64, 65):
        solo("size_%d" % n, "a buffer of %d bytes%s" % (n, {0: ": one empty raw block", 63: ": below the block forms' 64", 64: ": blen >= 64, nl >= 64"}.get(n, "")),
             low4(dc._rng("size%d" % n), n), ["size_%d" % n], lambda v, n=n: len(v.p) == n and len(v.pieces) == 1)
    for n in (16383, 16384, 16385, 32768, 32769):
        rec("size_%d" % n, "a payload of %d bytes: blocks of %s" % (n, " + ".join(str(len(x)) for x in zenc_pieces(bytes(n)))), ["size_%d" % n],
            lambda v, n=n: len(v.p) == n and [len(x) for x in v.pieces] == [len(x) for x in zenc_pieces(bytes(n))], plen=n, runs=[(5000, 5)])
    big = bytearray((1 << 24) + 5)
    for at in (3, 9000, ZBLOCK * 700 + 5, (1 << 24) + 4):
        big[at] = 0x55
    solo("size_16777221", "2^24 + 5 zero bytes with four planted literals: the content size's fourth byte is 1 (z.carry = plen >> 24), 1025 blocks, most of them RLE",
         big, ["size_16777221_carry_byte"], lambda v: len(v.p) >> 24 == 1 and len(v.pieces) == 1025 and len(v.pieces[-1]) == 5)
    # ---- block choice
    solo("rle_block_64", "64 equal bytes: one run, nseq == 1 && nlit == 1 refuses the sequence, and the block is an RLE block", X * 64, ["rle_block"],
         lambda v: v.tok[0][1] == [(1, 63)] and not v.tok[0][2] and v.distinct() == 1)
    solo("literal_then_run", "one literal and a run of 99: the sequence is taken, a compressed block with two raw literals", b"\x01" + X * 99,
         ["literal_then_run_two_raw_literals", "nseq_1"], lambda v: v.tok[0] == (b"\x01\xe0", [(2, 98)], True))
    solo("run_63", "63 equal bytes: below 64 neither sequences nor an RLE block, a raw block", X * 63, ["run_63_raw"], lambda v: not v.tok[0][2] and len(v.p) == 63)
    solo("incompressible_200", "200 different byte values: an optimal code needs more than 200 bytes with its description, a raw block",
         bytes(dc._rng("inc200").permutation(256)[:200].astype(np.uint8)), ["incompressible_raw"],
         lambda v: v.distinct() == 200 and not v.tok[0][2] and raw_is_pinned(v.p))
    solo("flat_256_x_32", "every byte value 32 times: all code lengths 8, ONE weight value, which the FSE form cannot say (zstd_desc_head returns 0): a raw block",
         dc.flat_bytes(dc._rng("flat"), 8192), ["flat_single_weight_raw"],
         lambda v: set(v.hist()) == {32} and not v.tok[0][2] and set(shannon_clamped(v.hist())) == {8} and raw_is_pinned(v.p))
    # use = ... && nlit + 4 nseq + 8 <= blen && 3 + nlit + 4 + ((12 nseq + nlit / 4 + (blen - nlit) / 8 + 20) >> 3) + 1 < blen
    ten = lambda last: b"".join(bytes([0xE0 + i]) * 5 for i in range(9)) + bytes([0xE9]) * last
    solo("use_first_refuses", "ten runs, nine of 5 and one of 12, behind 143 literals: blen - nlit = 4 nseq + 7, one short of the room for the sequence records",
         bgs("u1", 143) + ten(12), ["use_first_inequality_refuses"],
         lambda v: len(v.tok[0][1]) == 10 and not v.tok[0][2] and len(v.p) - len(v.tok[0][0]) == 47 and use_terms(v.p) == (False, True))
    solo("use_first_takes", "the same with a run of 13: blen - nlit = 4 nseq + 8", bgs("u1", 143) + ten(13), ["use_first_inequality_takes"],
         lambda v: len(v.tok[0][1]) == 10 and v.tok[0][2] and len(v.p) - len(v.tok[0][0]) == 48 and use_terms(v.p) == (True, True))
    solo("use_second_takes", "58 literals and a run of 15: 3 + 59 + 4 + (47 >> 3) + 1 = 72 < 73", bgs("u2", 58) + X * 15, ["use_second_inequality_takes"],
         lambda v: v.tok[0][1] == [(59, 14)] and v.tok[0][2] and use_terms(v.p) == (True, True))
    solo("use_second_refuses", "59 literals and a run of 15: 3 + 60 + 4 + (48 >> 3) + 1 = 74, not < 74", bgs("u2", 59) + X * 15, ["use_second_inequality_refuses"],
         lambda v: v.tok[0][1] == [(60, 14)] and not v.tok[0][2] and use_terms(v.p) == (True, False))
    # ---- tokeniser geometry
    long_id = b"\x01" * 3 + b"craftcraf" * 28 + b"cr"                        # 257 bytes: id length 01 01, then 01 01 01: a run of 5 from position 0
    assert len(long_id) == 257
    for K, blen in ZENC_KS:
        assert zenc_chunk(blen) == K and blen % K
        c = 80 // K + 2                                                      # a lane chunk behind the head
        g = lambda x, K=K: ["k%d_%s" % (K, x)]
        rec("k%d_runs_4_5_6" % K, "K = %d (blen %d): runs of exactly 4, 5 and 6 — the first is no sequence" % (K, blen), g("runs_4_5_6"),
            lambda v, c=c, K=K: [x[1] for x in v.tok[0][1][5:]] == [4, 5] and v.has_run(c * K + 1, 4) and v.has_run((c + 9) * K + 1, 5) and v.has_run((c + 18) * K + 1, 6),
            plen=blen, runs=[(c * K + 1, 4), ((c + 9) * K + 1, 5), ((c + 18) * K + 1, 6)])
        rec("k%d_run_from_last_byte" % K, "K = %d: a run of 6 whose first byte is the last of a lane chunk: the lane sees one break and nothing behind it" % K,
            g("run_from_last_byte_of_chunk"), lambda v, c=c, K=K: v.has_run(c * K + K - 1, 6), plen=blen, runs=[(c * K + K - 1, 6)])
        rec("k%d_run_from_k_minus_5" % K, "K = %d: a run of 5 from chunk offset K - 5: the last start whose RMIN - 1 followers lie inside the chunk" % K,
            g("run_from_chunk_offset_k_minus_5") + g("run_ends_on_chunk_end"), lambda v, c=c, K=K: v.has_run(c * K + K - 5, 5),
            plen=blen, runs=[(c * K + K - 5, 5)])
        rec("k%d_run_from_k_minus_4" % K, "K = %d: a run of 5 from chunk offset K - 4: its last byte is the next lane's first" % K,
            g("run_from_chunk_offset_k_minus_4"), lambda v, c=c, K=K: v.has_run(c * K + K - 4, 5), plen=blen, runs=[(c * K + K - 4, 5)])
        rec("k%d_run_ends_on_chunk_end" % K, "K = %d: a run of 7 whose last byte is the last of a lane chunk" % K, g("run_ends_on_chunk_end"),
            lambda v, c=c, K=K: v.has_run((c + 2) * K - 7, 7), plen=blen, runs=[((c + 2) * K - 7, 7)])
        rec("k%d_run_over_whole_chunks" % K, "K = %d: a run from the middle of one lane chunk over three whole ones into a fifth: lanes without a break" % K,
            g("run_over_whole_chunks"), lambda v, c=c, K=K: v.has_run(c * K + 2, 4 * K), plen=blen, runs=[(c * K + 2, 4 * K)])
        rec("k%d_run_across_wave" % K, "K = %d: a run of 8 from lane 63 into lane 64: the break positions cross the waves through S.ws" % K,
            g("run_across_wave_boundary"), lambda v, K=K: v.has_run(64 * K - 3, 8), plen=blen, runs=[(64 * K - 3, 8)])
        rec("k%d_run_spans_a_wave" % K, "K = %d: a run from lane 62 to lane 130: a whole wave without a break" % K, g("run_spans_a_wave"),
            lambda v, K=K: v.has_run(62 * K + 1, 68 * K + 1), plen=blen, runs=[(62 * K + 1, 68 * K + 1)])
        rec("k%d_run_from_position_0" % K, "K = %d: a run of 5 from position 0 (id length 257 = 01 01, the read id starts 01 01 01)" % K, g("run_from_position_0"),
            lambda v: v.runs[0][0] == (0, 5) and v.tok[0][1][0] == (1, 4), plen=blen, read_id=long_id)
        rec("k%d_run_to_the_end" % K, "K = %d: a block of %d bytes — lane %d holds %d bytes, the lanes behind it none — that ends in a run of 9" %
            (K, blen, blen // K, blen % K), g("run_to_block_end") + g("partial_last_lane"),
            lambda v, blen=blen, K=K: len(v.p) == blen and v.has_run(blen - 9, 9) and 0 < blen % K and blen // K < 255, plen=blen, runs=[(blen - 9, 9)])
    # bytes behind a short last block.  The staged kernel copies a block in 16-byte units, so what the tokeniser's last dword holds behind blen
    # is never the block staged before (that would be the first thought) but the slot memory behind the parked payload: STALE_FILL is what the
    # GPU tests put there — byte E5, the runs', right behind the payload, another value behind that.  A break bit behind blen does harm in two
    # places: in the lane where a run starts that reaches the block's end (its `hi`), and in lane 255, whose first break the lanes in front take
    # for the end of their run (behind any other lane an idle lane says blen)
    def stale_aux(h):
        pay = bytearray(h) + dc.background(dc._rng("zenc:stale"), ZBLOCK + 1030 - h)
        pay[ZBLOCK + 100:ZBLOCK + 300] = b"\xe6" * 200
        pay[ZBLOCK + 1025:] = b"\xe5" * 5
        return bytes(pay[h:])
    rec("stale_bytes_behind_short_block", "16384 + 1030 bytes (K = 8): the second block ends in a run of five E5 that starts in its last lane, two bytes short of that lane's "
        "second dword; the two bytes behind it are whatever lies behind the parked payload (the tests fill the slots: E5, then 00).  Only the `valid` mask keeps the run at five",
        ["stale_bytes_behind_short_second_block"],
        lambda v: len(v.pieces[1]) == 1030 and zenc_chunk(1030) == 8 and v.runs[1][-1] == (1025, 5) and 1025 // 8 == 1029 // 8 and v.tok[1][1][-1][1] == 4 and v.tok[1][2]
        and STALE_FILL[len(v.p) % 4:len(v.p) % 4 + 2] == b"\xe5\x00", aux=stale_aux)
    def stale_aux(h):
        pay = bytearray(h) + dc.background(dc._rng("zenc:stale255"), 16382 - h)
        pay[1000:3000] = b"\xe6" * 2000
        pay[16266:] = b"\xe5" * 116
        return bytes(pay[h:])
    rec("stale_bytes_behind_lane_255", "16382 bytes (K = 64): a run of 116 bytes E5 from lane 254 to the block's end in lane 255, which holds 62 bytes and no break; the "
        "two bytes behind are the slot's (E5, then 00): a break there would be the first that the lanes in front see", ["stale_bytes_behind_last_lane"],
        lambda v: len(v.p) == 16382 and zenc_chunk(16382) == 64 and v.runs[0][-1] == (16266, 116) and 16266 // 64 == 254 and v.tok[0][1][-1][1] == 115 and v.tok[0][2]
        and STALE_FILL[len(v.p) % 4:len(v.p) % 4 + 2] == b"\xe5\x00", aux=stale_aux)
    # ---- sequences
    for n in (63, 64, 65, 127, 128, 129):
        rec("nseq_%d" % n, "%d sequences (five of them in the head): the count's byte width, the sequences wave's passes of 64" % n, ["nseq_%d" % n],
            lambda v, n=n: len(v.tok[0][1]) == n and v.tok[0][2], plen=80 + 13 * (n - 5), runs=[(70 + 13 * i, 5) for i in range(n - 5)])
    most = b"".join(bytes([0xE0 + i % 16]) * 5 for i in range(3274)) + b"\x7a" + b"\x7b" * 13
    solo("nseq_most", "3274 runs of 5, a literal and a run of 13: 3275 sequences and 3276 literals, nlit + 4 nseq + 8 = 16384 exactly — the most a block admits, the "
         "sequence records fill the stage to its last word", most, ["nseq_3275"],
         lambda v: len(v.p) == ZBLOCK and len(v.tok[0][1]) == 3275 and len(v.tok[0][0]) == 3276 and v.tok[0][2] and use_terms(v.p) == (True, True)
         and not zenc_tokens(b"".join(bytes([0xE0 + i % 16]) * 5 for i in range(3276)))[2])
    def ll_aux(h):
        out = bytearray(X * 1500)                                            # (matched bytes enough for `use` to take the block)
        rng = dc._rng("zenc:ll")
        for i, ll in enumerate(ZENC_LL_STEPS):
            out += dc.background(rng, ll - 1) + bytes([0xE1 + i % 2]) * 6
        return bytes(out)
    rec("ll_steps", "literal lengths %s: both sides of every step of zstd_ll_code" % ", ".join(map(str, ZENC_LL_STEPS)), ["ll_%d" % n for n in ZENC_LL_STEPS],
        lambda v: [x[0] for x in v.tok[0][1][-len(ZENC_LL_STEPS):]] == list(ZENC_LL_STEPS) and v.tok[0][2]
        and [ll_code(n) for n in ZENC_LL_STEPS] == [15, 16, 19, 20, 21, 22, 23, 24, 24, 25, 25, 26, 31], aux=ll_aux)
    def ml_aux(h):
        out = bytearray()
        for i, mb in enumerate(ZENC_MB_STEPS[:-1]):
            out += b"abc" + bytes([0xE0 + i % 2]) * (mb + 4)
        return bytes(out)
    rec("ml_steps", "match lengths of mb + 3 for mb = %s: both sides of every step of zstd_ml_code" % ", ".join(map(str, ZENC_MB_STEPS[:-1])),
        ["mb_%d" % n for n in ZENC_MB_STEPS[:-1]],
        lambda v: [x[1] - 3 for x in v.tok[0][1][-14:]] == list(ZENC_MB_STEPS[:-1]) and v.tok[0][2]
        and [ml_code(n + 3) for n in ZENC_MB_STEPS[:-1]] == [31, 32, 35, 36, 37, 38, 39, 40, 41, 42, 42, 43, 43, 44], aux=ml_aux)
    solo("ml_longest", "one literal and a run of 16383: the longest match a block can hold, 16382 = mb 16379, code 49 with 13 extra bits", b"\x01" + X * 16383,
         ["mb_16379"], lambda v: v.tok[0] == (b"\x01\xe0", [(2, 16382)], True) and ml_code(16382) == 49 and ML_BITS[49] == 13)
    # ---- literals section
    for nl in (31, 32):
        solo("seq_raw_literals_%d" % nl, "%d literals beside a sequence: nl < 64, raw literals with a %d-byte header" % (nl, 1 if nl < 32 else 2),
             bgs("rl%d" % nl, nl - 1) + X * 40, ["seq_raw_literals_%d" % nl], lambda v, nl=nl: len(v.tok[0][0]) == nl and v.tok[0][2])
    for nl in (4095, 4096):
        flat = b"".join(bytes(dc._rng("rl%d" % i).permutation(256).astype(np.uint8)) for i in range(16))
        solo("seq_raw_literals_%d" % nl, "%d literals of every value about equally often beside a sequence: no code beats 8 bits, raw literals with a %d-byte header" %
             (nl, 2 if nl < 4096 else 3), flat[:nl - 1] + X * 300, ["seq_raw_literals_%d" % nl],
             lambda v, nl=nl: len(v.tok[0][0]) == nl and v.tok[0][2] and len(v.tok[0][1]) == 1 and huffman_floor(v.lits[0]) >= nl + 3)
    for nl, what in ((64, "the least the Huffman form takes: streams of 16 literals, a lane holds at most one"), (65, "streams of 17, 17, 17 and 14: an uneven last stream"),
                     (1023, "the 3-byte header's last"), (1024, "the 4-byte header's first"), (16383, "the 4-byte header's last"), (16384, "the 5-byte header")):
        solo("huf_nl_%d" % nl, "%d literals over four values, no run: %s" % (nl, what), low4(dc._rng("hnl%d" % nl), nl), ["huf_nl_%d" % nl],
             lambda v, nl=nl: len(v.lits[0]) == nl and not v.tok[0][2] and v.distinct() == 4 and huffman_is_pinned(v.p))
    near = bytes(dc._rng("near").permutation(np.repeat(np.arange(200, dtype=np.uint8), [12] * 23 + [4] * 177))[:983])
    solo("huf_csize_near_1023", "983 literals of 200 values beside a run of 60: csize comes out near nl, far from the 1023 it would have to pass with nl below it — kept "
         "Huffman literals have csize < nl, so that side of `csize <= 1023` cannot be reached (see the catalogue's docstring)", near + X * 60, ["huf_csize_near_1023"],
         lambda v: len(v.tok[0][0]) == 984 and v.tok[0][2])
    # ---- code lengths
    solo("distinct_2", "two values, 3 and 250, no run of five: the exact construction; 250 weights of which one is not zero", bytes(dc.background(dc._rng("d2"), 3000, b"\x03\xfa")),
         ["distinct_2"], lambda v: v.distinct() == 2 and v.maxsym() == 250)
    for k in (16, 17):
        p = 0.8 ** np.arange(k)
        x = dc._rng("d%d" % k).choice(k, 3000, p=p / p.sum())
        for i in range(3, 3000):
            if x[i] == x[i - 1] == x[i - 2] == x[i - 3]:
                x[i] = (x[i] + 1) % k
        body = bytes(0x30 + int(a) for a in x)
        solo("distinct_%d" % k, "%d values of geometric frequencies: %s" % (k, "the last alphabet of the exact construction" if k == 16 else "the first of the tree-free one"),
             body, ["distinct_%d" % k], lambda v, k=k: v.distinct() == k and not v.tok[0][1])
    geo = {0x10 + i: 8192 >> i for i in range(11)}
    geo.update({0xC0 + i: 1 for i in range(8)})
    solo("geometric_and_eight_singles", "frequencies 8192, 4096 .. 8 and eight values seen once, the last of them 199: the Shannon lengths clamped to 11 bits over-subscribe the "
         "code space, assign_lengths_wave gives up and the exact construction repairs the Kraft sum; 199 weights, most weight values seen once: their normalised counts "
         "sum above 64", spread(geo), ["clamp_oversubscribes", "normalise_takes"],
         lambda v: v.distinct() == 19 and not v.tok[0][1] and kraft(shannon_clamped(v.hist())) == (1 << 11) + 7 and max(dc.shannon_lengths(v.hist())) == 14)
    dy = {0x10 + i: 8192 >> i for i in range(11)}
    dy[140] = 8
    solo("dyadic_12_longest_11", "frequencies 8192, 4096 .. 8, 8 (the last for value 140): any code within the Shannon bound has lengths 1 .. 10, 11, 11; twelve values, the "
         "exact construction; 140 weights, each weight 1 .. 11 listed once beside 129 zeros: 58 + 11 normalised counts, five to take back", spread(dy),
         ["longest_code_11_exact", "normalise_takes"],
         lambda v: v.distinct() == 12 and max(v.forced_weights()) == 11 and sorted(v.forced_weights())[-11:] == list(range(1, 12)) and normalise_sum(v.forced_weights()) == 69)
    dy = {0x80 + i: 512 for i in range(16)}
    dy.update({0x10 + i: 4096 >> i for i in range(10)})
    dy[0x40] = 8
    solo("dyadic_27_longest_11", "sixteen values 512 times, then 4096, 2048 .. 8, 8: 27 values, the tree-free construction with no slack to hand out, longest code 11",
         spread(dy), ["longest_code_11_tree_free", "normalise_takes"],
         lambda v: v.distinct() == 27 and max(v.forced_weights()) == 10 and min(w for w in v.forced_weights() if w) == 1 and normalise_sum(v.forced_weights()) == 68)
    dy = {0x20: 8192, 250: 128}
    dy.update({0x60 + i: 256 for i in range(20)})
    dy.update({0x80 + i: 128 for i in range(23)})
    solo("dyadic_45_normalise_gives", "one value of 1 bit, 20 of 6 and 24 of 7, the last of them 250: of 250 weights 206 are 0, 23 are 1, 20 are 2 and one is 7 — normalised "
         "52 + 5 + 5 + 1 = 63, and the largest count is given the missing one", spread(dy), ["normalise_gives"],
         lambda v: v.distinct() == 45 and weight_counts(v.forced_weights()) == [206, 23, 20, 0, 0, 0, 0, 1] and normalise_sum(v.forced_weights()) == 63)
    # ---- tree description
    for top in (127, 128, 129):
        solo("maxsym_%d" % top, "four small values and value %d: %d weights listed, %s" % (top, top, "the first FSE form" if top > 128 else "direct nibbles, an %s count" %
             ("odd" if top & 1 else "even, the last direct form")), low4(dc._rng("ms%d" % top), 400) + bytes([top, 1, top, 2]) * 8,
             ["maxsym_%d" % top] + (["weights_odd"] if top == 127 else ["weights_even"] if top == 128 else []),
             lambda v, top=top: v.maxsym() == top and not v.tok[0][1] and huffman_is_pinned(v.p))
    # (one value of 1 bit and m = 2^(L - 1) of L bits: weights 0, 1 and L in use, L - 2 values between; 255 other values end that at L = 8, a gap of 6)
    for gap, L, m in ((1, 3, 4), (3, 5, 16), (4, 6, 32), (6, 8, 128)):
        dy = {0x20: 8192}
        dy.update({(0xA0 if m <= 32 else 0x60) + i: 8192 // m for i in range(m)})
        solo("fse_gap_%d" % gap, "one value half of the bytes, %d values the rest: weights 0, 1 and %d in use, %d weight values unused between: the count header's "
             "zero-run flag %s" % (m, L, gap, {1: "0", 3: "2", 4: "3 then 0", 6: "3 then 2"}[gap]), spread(dy), ["fse_gap_%d" % gap],
             lambda v, gap=gap: v.maxsym() > 128 and weight_gaps(v.forced_weights()) == [gap])
    # ---- output alignment
    for k in range(4):
        rec("align_phase_%d" % k, "two blocks; the first is %d literals and one long run, raw literals: its size grows by one with each of these four entries, so the second "
            "block's header, literals, jump table and sequences start at every byte phase of a word" % (33 + k), ["align_phase_%d" % k],
            lambda v, k=k: len(v.tok[0][0]) == 33 + k and len(v.tok[0][1]) == 6 and v.tok[0][2] and v.tok[1][2] and len(v.tok[1][0]) > 2000
            and v.tok[0][1][-1] == (9 + k + 3, ZBLOCK - 64 - k - 3) and ll_code(12) == 12 and ll_code(15) == 15 and ml_code(ZBLOCK - 70) == 49,
            aux=lambda h, k=k: bgs("al", 5)[:k + 2] + X * (ZBLOCK - h - k - 2) + bgs("al2", 1200) + Y * 200 + bgs("al3", 1800))
    # ---- literals-only mode (option zstd_sequences = 0): the split of an svb-zd record in the fused kernel
    walk = lambda name, n: np.cumsum(dc._rng("zenc:" + name).integers(-9, 10, n)).astype(np.int16) + 500
    for k in range(4):
        rid = b"craft0001xyz"[:9 + k]
        rec("lo_head_align_%d" % k, "an id of %d bytes: hdr_len + 12 = %d = %d mod 4 — in literals-only mode the raw head block ends, and the key and the data block "
            "start, there in LDS" % (9 + k, 59 + k, (59 + k) % 4), ["lo_head_align_%d" % k],
            lambda v, k=k: zenc_split(47 + k, 2000, len(v.p)) is not None and zenc_split(47 + k, 2000, len(v.p))[0] % 4 == (59 + k) % 4,
            aux=bgs("lo%d" % k, 100), signal=walk("lo%d" % k, 2000), read_id=rid)
    for at, ns in ((255, 784), (256, 788)):
        rec("lo_at_%d" % at, "%d samples: the key bytes end at %d — %s" % (ns, at, "no split below 256" if at < 256 else "the first split"), ["lo_at_%d" % at],
            lambda v, at=at, ns=ns: 59 + ((ns + 3) >> 2) == at and (zenc_split(47, ns, len(v.p)) is None) == (at < 256) and len(v.p) > at + 256,
            aux=b"", signal=walk("lo_at", ns))
    for tail in (255, 256):
        rid = b"craft0001" + b"x" * 201
        sig = walk("lo_tail", 100)
        h = len(head_of(tuple(sig), rid, dc.FIELDS2))
        at = 2 + 210 + 36 + 12 + 25
        rec("lo_tail_%d" % tail, "an id of 210 bytes and 100 samples: %d bytes behind the key bytes — %s" % (tail, "no split" if tail < 256 else "the shortest data block of a split"),
            ["lo_tail_%d" % tail], lambda v, tail=tail, at=at: len(v.p) - at == tail and (zenc_split(248, 100, len(v.p)) is None) == (tail < 256),
            aux=bgs("lot", 300)[:tail - (h - at)], signal=sig, read_id=rid)
    assert len({e["name"] for e in E}) == len(E)
    return E


def use_terms(block):
    """the two inequalities of `use`, each on its own, for a block with sequences"""
    lits, seqs, _ = zenc_tokens(block)
    blen, nlit, nseq = len(block), len(lits), len(seqs)
    return (nlit + 4 * nseq + 8 <= blen, 3 + nlit + 4 + ((12 * nseq + (nlit >> 2) + ((blen - nlit) >> 3) + 20) >> 3) + 1 < blen)


def huffman_floor(lits):
    """bytes that NO Huffman literals section of these literals goes below: a 3-byte header, the description (direct: 1 + ceil(n / 2) for n =
    the largest value in use, up to 128; FSE: at least 3), the jump table, and the four streams — together at least (bits + 4) / 8 bytes for the
    bits of an optimal 11-bit-limited code, each stream carrying its end mark"""
    h = histogram(lits)
    n = max(s for s, f in enumerate(h) if f)
    bits = code_bits(h, limited_lengths(h))
    return 3 + (1 + (n + 1) // 2 if n <= 128 else 3) + 6 + (bits + 4 + 7) // 8


def huffman_ceiling(lits):
    """bytes that the encoder's own Huffman literals section stays within when the clamped Shannon lengths are a code (which it only
    shortens): a 5-byte header, the description (direct: 1 + ceil(n / 2); FSE: at most 128 bytes), the jump table, the streams at the Shannon start with a byte of rounding each"""
    h = histogram(lits)
    sl, n = shannon_clamped(h), max(s for s, f in enumerate(h) if f)
    assert kraft(sl) <= 1 << ZMAXBITS
    return 5 + (1 + (n + 1) // 2 if n <= 128 else 128) + 6 + code_bits(h, sl) // 8 + 4


def raw_is_pinned(block):
    """a block without sequences of which the arithmetic alone says: raw (no Huffman section could make `hl + csize + 1 < blen` true)"""
    return len(block) < 64 or (not zenc_tokens(block)[2] and len(set(block)) > 1 and huffman_floor(block) + 1 >= len(block))


def huffman_certain(lits, blen):
    """a block without sequences whose own Huffman section the encoder must have found small enough (`hl + csize + 1 < blen`), whatever
    lengths it chose"""
    return len(lits) >= 64 and len(set(lits)) > 1 and kraft(shannon_clamped(histogram(lits))) <= 1 << ZMAXBITS and huffman_ceiling(lits) + 1 < blen


def huffman_is_pinned(block):
    """... and of which the arithmetic says: compressed, with Huffman literals"""
    return not zenc_tokens(block)[2] and huffman_certain(block, len(block))


def zenc_family(name):
    """the name with its numbers taken out: the entries of one loop of the catalogue"""
    return re.sub(r"\d+", "#", name)
