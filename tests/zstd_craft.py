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
"""
import collections
import os
import struct
import sys

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
    return Crafted(data, bytes(B.out) if B.ok else None, frozenset(B.tags | set(tags)) if B.ok else frozenset())


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
