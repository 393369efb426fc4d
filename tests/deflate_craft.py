"""Hand-made DEFLATE for the inflate tests (test infrastructure; STOCK zlib is the referee of what is valid — RFC 1950 / 1951).

Two layers.  The first (dynamic_block, zlib_stream, raw_stream_with_sequence: the header tests of test_gpu_parity.py) writes one dynamic
block of literals and varies its HEADER:

  lit/len code lengths   chosen by the caller (any complete canonical code)
  sequence tokens        "plain": one token per length, "rle": zlib-like runs, "rep0": symbol 16 behind zero lengths as well
  code-length code       from the token frequencies (Huffman, limited to 7 bits), or from caller's weights (shapes with 1-bit codes)

The second (Stream, py_inflate, catalogue; tests/test_inflate_craft.py) writes whole streams token by token — stored, fixed and dynamic
blocks at any bit offset, any symbol and extra-bit choice, any code lengths, complete or not, any zlib wrapper — executes its own tokens to
know what a valid stream holds, and restates inflate in plain Python from the RFCs, with zlib's rules for the code tables.
"""
import collections
import functools
import heapq
import struct
import zlib

import numpy as np

ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nb):                     # nb bits of v, least significant first
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nb):             # a Huffman code: first bit of the code first
        if nb:
            self.put(int(format(code, "0%db" % nb)[::-1], 2), nb)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def huff_lengths(weights, limit):
    """code lengths of a Huffman code over the symbols with weight > 0 (at least two), every length <= limit (asserted: the callers
    choose weights that fit); a complete code"""
    live = [(w, i) for i, w in enumerate(weights) if w > 0]
    assert len(live) >= 2
    heap = [(w, i, (i,)) for w, i in live]
    heapq.heapify(heap)
    depth = [0] * len(weights)
    tick = len(weights)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    assert max(depth) <= limit, (max(depth), limit)
    return depth


def canonical(lengths):
    """RFC 1951 3.2.2: code of every symbol (None for length 0)"""
    bl = [0] * 17
    for l in lengths:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def tokens_of(seq, mode):
    """the code-length sequence as (symbol, extra value) tokens.  plain: one token per length; rle: zero runs as 18 / 17, other runs as the
    length followed by 16s (what zlib writes); rep0: zero runs ALSO as "0, then 16s" (a repeat of a zero length: legal, zlib never writes it)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        j = i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if mode == "plain":
            out += [(v, 0)] * run
        elif v == 0 and mode == "rle":
            while run >= 11:
                r = min(run, 138); out.append((18, r - 11)); run -= r
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                r = min(run, 6); out.append((16, r - 3)); run -= r
            out += [(v, 0)] * run
        i = j
    return out


def dynamic_block(payload, litlens, mode="rle", cl_weights=None, final=True, dlens=(1, 1)):
    """one dynamic block of literals: payload bytes under the lit/len code `litlens` (>= 257 entries, complete, every used byte and
    symbol 256 with a length), distance code lengths dlens"""
    assert len(litlens) >= 257 and len(litlens) <= 286 and litlens[256]
    seq = list(litlens) + list(dlens)
    toks = tokens_of(seq, mode)
    freq = [0] * 19
    for s, _ in toks:
        freq[s] += 1
    if cl_weights is not None:
        w = [cl_weights.get(s, 0) for s in range(19)]
        assert all(w[s] > 0 for s in range(19) if freq[s])
    else:
        w = list(freq)
    if sum(1 for x in w if x) < 2:
        w[[s for s in range(19) if not w[s]][0]] = 1
    cll = huff_lengths(w, 7)
    clc = canonical(cll)
    hclen = 19
    while hclen > 4 and cll[ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(litlens) - 257, 5)
    b.put(len(dlens) - 1, 5)
    b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cll[ORDER[k]], 3)
    hdr_start = 3 + 14 + 3 * hclen
    nbits = 0
    for s, x in toks:
        b.put_code(clc[s], cll[s]); nbits += cll[s]
        if s == 16:
            b.put(x, 2); nbits += 2
        elif s == 17:
            b.put(x, 3); nbits += 3
        elif s == 18:
            b.put(x, 7); nbits += 7
    lc = canonical(list(litlens))
    for x in payload:
        assert litlens[x], "byte %d has no code" % x
        b.put_code(lc[x], litlens[x])
    b.put_code(lc[256], litlens[256])
    return b, hdr_start, nbits


def zlib_stream(payload, litlens, **kw):
    """-> (zlib stream, bits of the code-length sequence); checked against stock zlib"""
    b, _, nbits = dynamic_block(payload, litlens, **kw)
    s = b"\x78\x9c" + b.done() + struct.pack(">I", zlib.adler32(payload) & 0xFFFFFFFF)
    assert zlib.decompress(s) == payload
    return s, nbits


def raw_stream_with_sequence(toks, cll, hlit, hdist, tail_bits=64):
    """a zlib stream whose dynamic header carries exactly these (symbol, extra) tokens under the code-length code `cll` — for headers that
    are NOT valid (a repeat with nothing in front, a run over the end); nothing follows but zero bits and a dummy trailer"""
    clc = canonical(cll)
    hclen = 19
    while hclen > 4 and cll[ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = Bits()
    b.put(1, 1); b.put(2, 2); b.put(hlit - 257, 5); b.put(hdist - 1, 5); b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cll[ORDER[k]], 3)
    for s, x in toks:
        b.put_code(clc[s], cll[s])
        if s == 16:
            b.put(x, 2)
        elif s == 17:
            b.put(x, 3)
        elif s == 18:
            b.put(x, 7)
    b.put(0, tail_bits)
    return b"\x78\x9c" + b.done() + b"\x00\x00\x00\x01"


# ================================================================ whole streams, token by token
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8          # RFC 1951 3.2.6 (symbols 286 and 287 have codes and no meaning)
FIXED_DL = [5] * 32                                            # (so have distance symbols 30 and 31)


def lit(b):
    return ("lit", b)


def lits(data):
    return [("lit", x) for x in data]


def match(length, distance, lsym=None, lextra=None, dsym=None, dextra=None):
    """a match of `length` bytes from `distance` back.  The length symbol, the distance symbol and their extra bits default to the one
    choice an encoder makes; an override writes any other pair that the format allows (258 as symbol 284 + extra 31) or does not
    (distance symbols 30 and 31: no extra bits)."""
    if lsym is None:
        lsym = 285 if length == 258 else 257 + max(s for s in range(28) if LBASE[s] <= length)
    if lextra is None:
        lextra = length - LBASE[lsym - 257]
    if dsym is None:
        dsym = max(s for s in range(30) if DBASE[s] <= distance)
    if dextra is None:
        dextra = distance - DBASE[dsym] if dsym < 30 else 0
    if 257 <= lsym <= 285:
        assert 0 <= lextra < (1 << LEXT[lsym - 257]) and LBASE[lsym - 257] + lextra == length, (length, lsym, lextra)
    if dsym < 30:
        assert 0 <= dextra < (1 << DEXT[dsym]) and DBASE[dsym] + dextra == distance, (distance, dsym, dextra)
    return ("match", length, distance, lsym, lextra, dsym, dextra)


def sym(s, extra=0, nextra=0):
    """a lit/len symbol as given, with nextra extra bits behind it and nothing else (286, 287; a length symbol without its distance)"""
    return ("sym", s, extra, nextra)


def bits(value, nbits):
    """nbits bits as given, least significant first (the escape for what no token says)"""
    return ("bits", value, nbits)


def _codes(lengths):
    """(code with its first bit last — ready for Bits.put —, length) per symbol; None where the length is 0"""
    return [None if c is None else (int(format(c, "0%db" % l)[::-1], 2), l) for c, l in zip(canonical(list(lengths)), lengths)]


class Stream:
    """DEFLATE blocks written one behind the other into one bit stream, and the bytes their tokens produce.  `valid` turns False when a
    token is written that no decoder may accept (a distance in front of the output, a symbol without meaning); what the block HEADERS say
    is not judged here — the catalogue names such streams malformed itself.  marks: (bit position behind the token, bytes out) per token."""

    def __init__(self):
        self.b, self.out, self.valid, self.marks = Bits(), bytearray(), True, []

    @property
    def bitpos(self):
        return self.b.bitpos

    def _tokens(self, toks, lc, dc, eob):
        b, out = self.b, self.out
        for t in toks:
            if t[0] == "lit":
                b.put(*lc[t[1]])
                out.append(t[1])
            elif t[0] == "match":
                _, length, dist, ls, lx, ds, dx = t
                b.put(*lc[ls])
                b.put(lx, LEXT[ls - 257])
                b.put(*dc[ds])
                if ds < 30:
                    b.put(dx, DEXT[ds])
                if ds >= 30 or dist > len(out):
                    self.valid = False
                else:
                    for _ in range(length):
                        out.append(out[-dist])
            elif t[0] == "sym":
                b.put(*lc[t[1]])
                b.put(t[2], t[3])
                self.valid = False
            else:
                b.put(t[1], t[2])
            self.marks.append((b.bitpos, len(out)))
        if eob:
            b.put(*lc[256])
        return self

    def stored(self, data, final=False, nlen=None, length=None, pad=0):
        """header, `pad` in the bits up to the byte boundary, LEN (default len(data)), NLEN (default its complement), the bytes"""
        b = self.b
        b.put(1 if final else 0, 1)
        b.put(0, 2)
        if b.n:
            b.put(pad, 8 - b.n)
        ln = len(data) if length is None else length
        b.put(ln, 16)
        b.put((ln ^ 0xFFFF) if nlen is None else nlen, 16)
        assert b.n == 0
        b.out += data
        self.out += data
        self.marks.append((b.bitpos, len(self.out)))
        return self

    def fixed(self, toks, final=False, eob=True):
        self.b.put(1 if final else 0, 1)
        self.b.put(1, 2)
        return self._tokens(toks, _codes(FIXED_LL), _codes(FIXED_DL), eob)

    def dynamic(self, toks, litlens, dlens, final=False, mode="rle", cl_weights=None, cll=None, eob=True):
        """litlens: 257 .. 288 lengths (HLIT is a 5-bit field: 287 and 288 can be written, and are wrong), dlens: 1 .. 32 (HDIST likewise).
        The code-length code comes from the sequence's token frequencies, from cl_weights, or is given as `cll` (19 lengths, any)."""
        assert 257 <= len(litlens) <= 288 and 1 <= len(dlens) <= 32
        b = self.b
        seq = tokens_of(list(litlens) + list(dlens), mode)
        if cll is None:
            freq = [0] * 19
            for s, _ in seq:
                freq[s] += 1
            w = list(freq) if cl_weights is None else [cl_weights.get(s, 0) for s in range(19)]
            assert all(w[s] > 0 for s in range(19) if freq[s])
            if sum(1 for x in w if x) < 2:
                w[[s for s in range(19) if not w[s]][0]] = 1
            cll = huff_lengths(w, 7)
        clc = _codes(cll)
        hclen = 19
        while hclen > 4 and cll[ORDER[hclen - 1]] == 0:
            hclen -= 1
        b.put(1 if final else 0, 1)
        b.put(2, 2)
        b.put(len(litlens) - 257, 5)
        b.put(len(dlens) - 1, 5)
        b.put(hclen - 4, 4)
        for k in range(hclen):
            b.put(cll[ORDER[k]], 3)
        for s, x in seq:
            b.put(*clc[s])
            b.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self.tokens_at = b.bitpos
        return self._tokens(toks, _codes(litlens), _codes(dlens), eob)

    def raw(self, value, nbits):
        self.b.put(value, nbits)
        return self

    def body(self):
        b = self.b
        return bytes(b.out) + (bytes([b.acc & 255]) if b.n else b"")

    def zlib(self, cinfo=7, cm=8, flevel=2, fdict=0, fcheck=None, adler=None, tail=b""):
        """RFC 1950 around the blocks: CMF = cinfo << 4 | cm, FLG = flevel << 6 | fdict << 5 | FCHECK (default: the one that makes the header
        a multiple of 31), the big-endian Adler-32 (default: of the bytes the tokens produced), `tail` behind it"""
        cmf = (cinfo << 4) | cm
        flg = (flevel << 6) | (fdict << 5)
        flg |= (31 - (cmf * 256 + flg) % 31) % 31 if fcheck is None else fcheck
        ad = zlib.adler32(bytes(self.out)) & 0xFFFFFFFF if adler is None else adler
        return bytes([cmf, flg]) + self.body() + struct.pack(">I", ad) + tail


def fill_complete(given, fillers, n):
    """n code lengths (0: unused): the symbols of `given` (symbol -> length) keep theirs, the `fillers` share what is left of the code space
    as evenly as it divides, so that the code is complete"""
    left = 32768 - sum(1 << (15 - l) for l in given.values())
    assert left > 0 and fillers
    parts = [15 - k for k in range(15, -1, -1) if (left >> k) & 1]          # lengths of one code per set bit, shortest first
    assert len(parts) <= len(fillers), (len(parts), len(fillers))
    heapq.heapify(parts)
    while len(parts) < len(fillers):
        l = heapq.heappop(parts)
        if l == 15:
            heapq.heappush(parts, l)
            break
        heapq.heappush(parts, l + 1)
        heapq.heappush(parts, l + 1)
    parts = sorted(parts)
    assert len(parts) == len(fillers), "the code space does not divide into that many codes"
    out = [0] * n
    for s, l in given.items():
        out[s] = l
    for s, l in zip(fillers, parts):
        out[s] = l
    assert sum(1 << (15 - l) for l in out if l) == 32768
    return out


def pad_literals(nbits, lengths, rng):
    """literal tokens whose codes under `lengths` take exactly nbits bits (two literal code lengths without a common factor must exist)"""
    by = {}
    for s in range(256):
        if lengths[s]:
            by.setdefault(lengths[s], []).append(s)
    ls = sorted(by)
    for a in ls:
        for c in ls:
            if a < c and _gcd(a, c) == 1:
                for j in range(a):
                    if nbits - j * c >= 0 and (nbits - j * c) % a == 0:
                        pick = [c] * j + [a] * ((nbits - j * c) // a)
                        return [("lit", by[l][int(rng.integers(0, len(by[l])))]) for l in pick]
    raise AssertionError("cannot pad %d bits with literal lengths %s" % (nbits, ls))


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


# ---------------------------------------------------------------- inflate restated from the RFCs (Python integers and a bytearray)
class Refused(Exception):
    def __init__(self, status, reason):
        Exception.__init__(self, reason)
        self.status, self.reason = status, reason


class _Reader:
    """bits of `data`, least significant bit of each byte first.  strict: a bit behind the end is a refusal ("truncated", as a decoder that
    waits for more input sees it); padded: bits behind the end read as zero and `over()` tells — the device decoders' contract"""

    def __init__(self, data, padded):
        self.d, self.pos, self.n, self.padded = data, 0, 8 * len(data), padded

    def get(self, k):
        v = 0
        for i in range(k):
            p = self.pos
            if p < self.n:
                v |= ((self.d[p >> 3] >> (p & 7)) & 1) << i
            elif not self.padded:
                raise Refused(3, "truncated")
            self.pos = p + 1
        return v

    def over(self):
        return self.pos > self.n

    def check(self):
        if self.pos > self.n:
            raise Refused(3, "truncated")


def _table(lengths, kind):
    """{(length, code): symbol} of a canonical code, under zlib's rules (inflate_table): an over-subscribed code is refused; an incomplete
    one too, unless it is the lit/len or distance code and consists of a single 1-bit code (or, the distance code, of none)"""
    used = [l for l in lengths if l]
    space = sum(1 << (15 - l) for l in used)
    if space > 32768:
        raise Refused(2, "over-subscribed %s code" % kind)
    if space < 32768 and used and (kind == "code-length" or used != [1]):
        raise Refused(2, "incomplete %s code" % kind)
    if not used and kind == "code-length":
        raise Refused(2, "incomplete code-length code")
    return {(l << 16) | c: s for s, (c, l) in enumerate(zip(canonical(list(lengths)), lengths)) if l}


def _decode(rd, tab):
    """RFC 1951 3.2.2, bit by bit: the first length at which the bits read so far are a code (the reader's own loop, written out: this is
    where the time goes)"""
    code, d, n, pos = 0, rd.d, rd.n, rd.pos
    for l in range(1, 16):
        bit = 0
        if pos < n:
            bit = (d[pos >> 3] >> (pos & 7)) & 1
        elif not rd.padded:
            raise Refused(3, "truncated")
        pos += 1
        code = (code << 1) | bit
        s = tab.get((l << 16) | code)
        if s is not None:
            rd.pos = pos
            return s
    rd.pos = pos
    return None


class Inflated:
    """data: the bytes (None: refused, then status / reason say why and `produced` how many bytes were out by then); marks: (bit position in
    the deflate data behind the token, bytes out) per literal, match and stored block; blocks: the type of every block; end_bit: behind the
    last block; gap: bytes between the last block and the Adler-32 as `framing` places it"""
    data = None
    status = 0
    reason = ""
    produced = 0
    end_bit = 0
    gap = 0

    def __init__(self):
        self.marks, self.blocks = [], []


@functools.lru_cache(maxsize=None)          # (the tests ask about the same few hundred streams again and again; the result is read, never changed)
def py_inflate(stream, framing="zlib"):
    """RFC 1950 + 1951 on `stream`.  framing "zlib": the Adler-32 stands right behind the last block and nothing behind it; bits are read
    strictly.  framing "device": the contract of csrc/inflate_dev.h — the LAST four bytes are the Adler-32, the deflate data is what lies
    between the header and them, bits behind it read as zero and running over the end is noticed behind the block header, behind LEN / NLEN,
    behind the code-length code's lengths, behind the code-length sequence and behind every token (status 3), a wrong token or a wrong
    sequence in front of such a place being noticed first (status 2); the
    last block must end in the last byte of the deflate data (else the Adler-32 is not where the stream says: status 4).
    The status numbers are the device's: 1 header, 2 data, 3 truncated, 4 Adler-32."""
    r = Inflated()
    out = bytearray()
    dev = framing == "device"
    try:
        if dev and len(stream) < 6:
            raise Refused(3, "shorter than header and trailer")
        if len(stream) < 2:
            raise Refused(3, "truncated")
        cmf, flg = stream[0], stream[1]
        if (cmf & 15) != 8:
            raise Refused(1, "compression method is not 8")
        if (cmf >> 4) > 7:
            raise Refused(1, "window larger than 32 KiB")
        if (cmf * 256 + flg) % 31:
            raise Refused(1, "header check")
        if flg & 0x20:
            raise Refused(1, "preset dictionary")
        body = stream[2:len(stream) - 4] if dev else stream[2:]
        rd = _Reader(body, dev)
        while True:
            final, typ = rd.get(1), rd.get(2)
            rd.check()
            r.blocks.append(typ)
            if typ == 3:
                raise Refused(2, "block type 3")
            if typ == 0:
                rd.pos = (rd.pos + 7) & ~7
                ln, nl = rd.get(16), rd.get(16)
                rd.check()
                if (ln ^ 0xFFFF) != nl:
                    raise Refused(2, "stored block: NLEN is not the complement of LEN")
                at = rd.pos >> 3
                if rd.over() or at + ln > len(body):
                    raise Refused(3, "truncated")
                out += body[at:at + ln]
                rd.pos += 8 * ln
                r.marks.append((rd.pos, len(out)))
            else:
                if typ == 1:
                    lt, dt = _table(FIXED_LL, "lit/len"), _table(FIXED_DL, "distance")
                else:
                    nl, nd, ncl = rd.get(5) + 257, rd.get(5) + 1, rd.get(4) + 4
                    if nl > 286 or nd > 30:
                        raise Refused(2, "too many length or distance symbols")
                    cl = [0] * 19
                    for k in range(ncl):
                        cl[ORDER[k]] = rd.get(3)
                    try:
                        ct = _table(cl, "code-length")
                    except Refused:
                        rd.check()                 # (lengths from behind the end are no code: the end is what is wrong)
                        raise
                    lens = []
                    while len(lens) < nl + nd:
                        s = _decode(rd, ct)
                        if s is None:
                            raise Refused(2, "invalid code in the code-length sequence")
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise Refused(2, "repeat with nothing in front")
                            v, rep = lens[-1], 3 + rd.get(2)
                        elif s == 17:
                            v, rep = 0, 3 + rd.get(3)
                        else:
                            v, rep = 0, 11 + rd.get(7)
                        if len(lens) + rep > nl + nd:
                            raise Refused(2, "run over the end of the code-length sequence")
                        lens += [v] * rep
                    rd.check()
                    if lens[256] == 0:
                        raise Refused(2, "no end-of-block code")
                    lt, dt = _table(lens[:nl], "lit/len"), _table(lens[nl:], "distance")
                while True:
                    s = _decode(rd, lt)
                    if s is None:
                        raise Refused(2, "invalid literal/length code")
                    if s < 256:
                        rd.check()
                        out.append(s)
                    elif s == 256:
                        rd.check()
                        break
                    else:
                        if s > 285:
                            raise Refused(2, "literal/length symbol %d" % s)
                        length = LBASE[s - 257] + rd.get(LEXT[s - 257])
                        ds = _decode(rd, dt)
                        if ds is None:
                            raise Refused(2, "invalid distance code")
                        if ds >= 30:
                            raise Refused(2, "distance symbol %d" % ds)
                        dist = DBASE[ds] + rd.get(DEXT[ds])
                        if dist > len(out):
                            raise Refused(2, "distance %d with %d bytes out" % (dist, len(out)))
                        rd.check()
                        for _ in range(length):
                            out.append(out[-dist])
                    r.marks.append((rd.pos, len(out)))
            if final:
                break
        r.end_bit = rd.pos
        end = (rd.pos + 7) >> 3
        if dev:
            r.gap = len(body) - end
            if r.gap:
                raise Refused(4, "%d bytes between the last block and the trailer" % r.gap)
            trailer = stream[-4:]
        else:
            trailer = body[end:end + 4]
            if len(trailer) < 4:
                raise Refused(3, "truncated")
            if len(body) > end + 4:
                r.gap = len(body) - end - 4
                raise Refused(4, "%d bytes behind the Adler-32" % r.gap)
        if struct.unpack(">I", trailer)[0] != (zlib.adler32(bytes(out)) & 0xFFFFFFFF):
            raise Refused(4, "Adler-32")
        r.data = bytes(out)
    except Refused as e:
        r.status, r.reason = e.status, e.reason
    r.produced = len(out)
    return r


def referee(stream):
    """stock zlib's verdict: the bytes if it takes the stream to its end with nothing left over, else None"""
    d = zlib.decompressobj(15)
    try:
        out = d.decompress(stream)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


# ================================================================ the catalogue: the smallest stream per route or edge
# The shapes follow the decoders' constants: csrc/inflate_dev.h reads through a 2048-byte window into a 4096-byte ring that is flushed at
# 2048 pending bytes; csrc/inflate_par_dev.h takes 4 KiB of compressed bytes per round in up to 64 segments of at least 384 bits, resolves
# lit/len codes through a 9-bit root table and parks up to 768 waiting matches per round; csrc/inflate_simt_dev.h collects four output
# bytes per store.
Entry = collections.namedtuple("Entry", "name stream expected status why")
# expected: the bytes (valid) or None; status: what every full decoder reports (0 valid, 1 header, 2 data, 3 truncated, 4 Adler-32; None:
# the entry pins only "never status 0 with other bytes")

FLAT257 = [8] * 255 + [9, 9]                   # complete: 255 / 256 + 2 / 512
FLAT286 = [8] * 226 + [9] * 60                 # complete, every symbol in use
DIST30 = [4, 4] + [5] * 28                     # complete, 30 codes
ONE_PREFIX = fill_complete({256: 10, 257: 11, 258: 12, 259: 13, 260: 14, 261: 15, 262: 15}, list(range(256)), 263)   # literals <= 9 bits; one code of each length
                                                                                                    # 10 .. 14 and two of 15: all under ONE 9-bit prefix
SEG = 384                                      # bits of the parallel decoder's shortest segment


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _rb(rng, n, lo=0, hi=256):
    return bytes(rng.integers(lo, hi, n, dtype=np.uint8))


def _cl(d):
    return [d.get(s, 0) for s in range(19)]


def seg_stream(span):
    """a stream whose LAST block's tokens start `span` bits in front of the end of the deflate data (the bits a round of the parallel
    decoder divides into segments): a short fixed block that sets the bit offset, then a final fixed block of literals"""
    rng = _rng("seg%d" % span)
    nine = (-span - 13) % 8                       # the last block's tokens start at bit 13 + 8 a + 9 b
    st = Stream().fixed(lits(_rb(rng, 1, 0, 144) + _rb(rng, nine, 144, 256)))
    start = st.bitpos + 3
    pad = (span - 7) % 8
    st.fixed(lits(_rb(rng, (span - 7 - pad) // 8, 0, 144)), final=True)
    assert 8 * len(st.body()) - start == span, (span, 8 * len(st.body()) - start)
    return st


def _cut_base():
    """the stream that the `cut_*` entries are prefixes of, and the bit positions of its structures"""
    rng = _rng("cut")
    at = {}
    st = Stream()
    at["block_header"] = 1
    at["hlit_hdist_hclen"] = 9
    at["code_length_code_lengths"] = 17 + 7
    toks = lits(_rb(rng, 40)) + [match(100, 30), match(258, 17), lit(5)]
    st.dynamic(toks, FLAT286, DIST30, mode="plain")
    at["code_length_sequence"] = (17 + st.tokens_at) // 2
    at["literal"] = st.tokens_at + 3
    m = st.marks[39][0]                           # behind the last of the 40 literals: match(100, 30) = 8- or 9-bit code, 4 extra, 5-bit code, 3 extra
    lcode = FLAT286[257 + 22]
    at["length_code"] = m + 1
    at["length_extra"] = m + lcode + 1
    at["distance_code"] = m + lcode + 4 + 1
    at["distance_extra"] = m + lcode + 4 + 5 + 1
    at["end_of_block"] = st.marks[-1][0] + 1
    p = (st.bitpos + 3 + 7) & ~7
    at["stored_len"] = p + 3
    at["stored_nlen"] = p + 16 + 3
    at["stored_bytes"] = p + 32 + 8 * 50
    st.stored(_rb(rng, 100))
    at["fixed_block_token"] = st.bitpos + 3 + 8 * 4 + 2
    st.fixed(lits(_rb(rng, 20, 0, 144)) + [match(9, 3)], final=True)
    at["last_end_of_block"] = st.bitpos - 2
    assert st.valid
    return st, at


@functools.lru_cache(maxsize=None)
def catalogue():
    """[Entry]: valid streams with the bytes the builder got by executing its own tokens, then the malformed ones"""
    E = []

    def V(name, st, why, **zk):
        assert st.valid, name
        E.append(Entry(name, st.zlib(**zk), bytes(st.out), 0, why))

    def M(name, data, status, why):
        E.append(Entry(name, bytes(data), None, status, why))

    # ---- matches
    for k in range(29):
        rng = _rng("len%d" % k)
        lo, hi = LBASE[k], LBASE[k] + (1 << LEXT[k]) - 1
        V("len_sym_%d" % (257 + k), Stream().fixed(lits(_rb(rng, 40)) + [match(lo, 7, lsym=257 + k), lit(1), match(hi, 33, lsym=257 + k)], final=True),
          "length symbol %d with its smallest and its largest extra value" % (257 + k))
    rng = _rng("258")
    V("len_258_as_284_plus_31", Stream().fixed(lits(_rb(rng, 9)) + [match(258, 9, lsym=284, lextra=31)], final=True),
      "length 258 written as symbol 284 with extra 31 (no encoder does)")
    V("len_258_as_285", Stream().fixed(lits(_rb(rng, 9)) + [match(258, 9)], final=True), "length 258 as symbol 285")
    for k in range(30):
        rng = _rng("dist%d" % k)
        lo, hi = DBASE[k], DBASE[k] + (1 << DEXT[k]) - 1
        st = Stream()
        if hi > 5000:
            st.stored(_rb(rng, hi - 3))
            st.fixed(lits(_rb(rng, 3)) + [match(4, lo, dsym=k), match(5, hi, dsym=k)], final=True)
        else:
            st.fixed(lits(_rb(rng, hi)) + [match(4, lo, dsym=k), match(5, hi, dsym=k)], final=True)
        V("dist_sym_%d" % k, st, "distance symbol %d with its smallest and its largest extra value" % k)
    for d in (32506, 32507, 32767, 32768):
        for L in (3, 258):
            rng = _rng("far%d_%d" % (d, L))
            V("far_d%d_l%d" % (d, L), Stream().fixed(lits(_rb(rng, d)) + [match(L, d), lit(7), match(L, d)], final=True),
              "distance %d (stock zlib's encoder stops at 32506), length %d: the source is the first bytes of the output" % (d, L))
    for k in (1, 2, 3, 4, 5, 64, 258, 259, 2047, 2048, 2049, 4095, 4096, 4097):
        rng = _rng("eq%d" % k)
        V("dist_eq_out_%d" % k, Stream().fixed(lits(_rb(rng, k)) + [match(258 if k > 5 else 10, k)], final=True),
          "distance = the %d bytes out so far, exactly" % k)
    for d in (1, 2, 3, 4):
        for o in range(4):
            rng = _rng("ov%d%d" % (d, o))
            V("overlap_d%d_o%d" % (d, o), Stream().fixed(lits(_rb(rng, 4 + o)) + [match(d + 9, d), lit(0xEE), match(258, d)], final=True),
              "distance %d with a longer length (the match reads what it writes), at output offset %d mod 4" % (d, o))
    for d in (4095, 4096, 4097):
        rng = _rng("ring%d" % d)
        V("dist_%d" % d, Stream().fixed(lits(_rb(rng, 6000)) + [match(258, d), match(3, d), lit(1), match(31, d)], final=True),
          "distance %d: the source at the edge of the 4096-byte output ring (in it, or read back from memory)" % d)
    rng = _rng("spans")
    V("match_source_spans_block_boundary", Stream().fixed(lits(_rb(rng, 100))).fixed(lits(_rb(rng, 3)) + [match(50, 20)], final=True),
      "a match whose source starts in the block before and runs on into its own output")
    V("match_source_spans_stored_block", Stream().fixed(lits(_rb(rng, 30))).stored(_rb(rng, 20)).fixed([lit(9), match(60, 45)], final=True),
      "a match whose source starts in a Huffman block, crosses a stored block and ends in its own output")
    V("match_destination_spans_flush", Stream().fixed(lits(_rb(rng, 1900)) + [match(258, 1500), match(258, 1)] + lits(_rb(rng, 90)) + [match(258, 2100), match(200, 300)], final=True),
      "matches that are being written when 2048 bytes are pending in the ring")
    V("match_behind_stored_copies_it", Stream().stored(_rb(rng, 300)).fixed([match(258, 300), match(100, 42)], final=True),
      "a match as the first token behind a stored block, copying out of it")
    # ---- blocks
    V("empty_fixed_block", Stream().fixed([], final=True), "a final fixed block that holds the end-of-block code and nothing else")
    V("empty_dynamic_block_eob_only", Stream().dynamic([], [0] * 256 + [1], [0], final=True),
      "a dynamic block whose lit/len code is the single 1-bit end-of-block code (incomplete, and allowed), no distance code")
    for n in (1, 2, 40):
        rng = _rng("empty%d" % n)
        st = Stream()
        for _ in range(n):
            st.fixed([])
        V("empty_blocks_%d_then_data" % n, st.fixed(lits(_rb(rng, 50)) + [match(20, 10)], final=True), "%d empty non-final blocks, then data" % n)
    for ln in (0, 1, 65535):
        for k in range(8):
            rng = _rng("st%d_%d" % (ln, k))
            st = Stream().fixed(lits(_rb(rng, 2, 0, 144) + _rb(rng, (k - 2) % 8, 144, 256)))
            assert st.bitpos % 8 == k
            st.stored(_rb(rng, ln), pad=0xFF if k & 1 else 0).fixed(lits(_rb(rng, 3)) + [match(4, 2)], final=True)
            V("stored_len%d_bit%d" % (ln, k), st, "a stored block of LEN %d whose header starts at bit %d of a byte" % (ln, k))
    for k in (0, 5):
        rng = _rng("laststored%d" % k)
        st = Stream().fixed(lits(_rb(rng, 2, 0, 144) + _rb(rng, (k - 2) % 8, 144, 256)))
        assert st.bitpos % 8 == k
        V("final_stored_block_bit%d" % k, st.stored(_rb(rng, 37), final=True), "the stream ends with a stored block (header at bit %d of a byte): the trailer stands right behind its bytes" % k)
    V("final_stored_block_empty", Stream().fixed(lits(_rb(rng, 9))).stored(b"", final=True), "the stream ends with an empty stored block")
    rng = _rng("between")
    V("stored_between_huffman_blocks", Stream().fixed(lits(_rb(rng, 100)) + [match(30, 50)]).stored(_rb(rng, 500))
      .dynamic(lits(_rb(rng, 60)) + [match(258, 400), match(40, 690)], FLAT286, DIST30, final=True), "fixed block, stored block, dynamic block with matches into both")
    for name, nbytes in (("final_block_ends_on_a_byte", 18), ("final_block_ends_on_the_2048_window", 2048), ("final_block_ends_on_the_4096_window", 4096)):
        rng = _rng(name)
        st = Stream().fixed(lits(_rb(rng, nbytes - 8, 0, 144) + _rb(rng, 6, 144, 256)), final=True)     # 3 + 8 a + 9 * 6 + 7 bits
        assert st.bitpos == 8 * nbytes
        V(name, st, "the end-of-block code of the final block ends on the last bit of byte %d of the deflate data" % (nbytes - 1))
    ll48 = fill_complete({256: 15, 284: 15}, list(range(256)), 285)
    dl48 = fill_complete({29: 15}, list(range(29)), 30)
    for edge in (2048, 4096):
        rng = _rng("tok48_%d" % edge)
        st = Stream().stored(_rb(rng, 25000))
        e0 = st.bitpos                                 # the dynamic block starts here: the window of either decoder does (the parallel one's up to 3 bytes earlier)
        st.dynamic([], ll48, dl48, eob=False)
        lead = e0 + 8 * (edge - 50) - st.bitpos
        toks = pad_literals(lead, ll48, rng) + [match(227 + int(rng.integers(0, 31)), 24577 + int(rng.integers(0, 300))) for _ in range(16)]
        st._tokens(toks, _codes(ll48), _codes(dl48), True)
        st.fixed(lits(_rb(rng, 5)), final=True)
        V("token48_across_the_%d_window" % edge, st, "sixteen 48-bit tokens (15-bit code, 5 extra, 15-bit distance code, 13 extra) in a row, "
          "from 50 bytes in front of byte %d of the block's window to 46 behind it" % edge)
    # ---- codes
    rng = _rng("codes")
    V("hdist1_length0_literals_only", Stream().dynamic(lits(_rb(rng, 300)), FLAT257, [0], final=True), "HDIST = 1 with length 0: no distance code, literals only")
    V("single_distance_code_of_1_bit", Stream().dynamic(lits(_rb(rng, 30)) + [match(10, 4), lit(3), match(258, 4)], FLAT286, [0, 0, 0, 1], final=True),
      "one distance code of length 1 (incomplete, and allowed)")
    V("distance_codes_30_complete", Stream().dynamic(lits(_rb(rng, 2100)) + [match(5, DBASE[k]) for k in range(23)], FLAT286, DIST30, final=True),
      "30 distance codes (two of 4 bits, 28 of 5: as 30 codes of 5 bits the set is incomplete and refused — see distance_codes_30_of_5_bits)")
    dl15 = fill_complete({10: 15, 11: 15}, [k for k in range(30) if k not in (10, 11)], 30)
    V("distance_codes_of_15_bits", Stream().dynamic(lits(_rb(rng, 100)) + [match(9, 33), match(9, 64), match(20, 1), match(7, 49)], FLAT286, dl15, final=True),
      "distance codes of 15 bits (longer than any lookup table)")
    V("litlen_codes_up_to_9_bits", Stream().dynamic(lits(_rb(rng, 200)) + [match(30, 100), match(258, 1)], FLAT286, DIST30, final=True), "no lit/len code longer than the 9-bit root table")
    V("litlen_long_codes_under_one_prefix", Stream().dynamic(lits(_rb(rng, 200)) + [match(3 + k, 10 + k) for k in range(6)] + [lit(0)] + [match(8 - k, 5) for k in range(6)], ONE_PREFIX, DIST30, final=True),
      "one lit/len code of each length 10 .. 14 and two of 15, all under one 9-bit prefix, everything else <= 9 bits")
    many = {s: 10 + (i % 6) for i, s in enumerate(list(range(196, 256)) + list(range(257, 286)))}
    many[256] = 15
    llm = fill_complete(many, list(range(196)), 286)
    V("litlen_long_codes_under_many_prefixes", Stream().dynamic(lits(_rb(rng, 400)) + [match(LBASE[k], 50 + k) for k in range(29)] + lits(_rb(rng, 300, 190, 256)), llm, DIST30, final=True),
      "ninety lit/len codes of 10 .. 15 bits: second-level tables of every size")
    st = Stream().dynamic([], ONE_PREFIX, DIST30, eob=False)
    t0 = st.bitpos
    lc, dc = _codes(ONE_PREFIX), _codes(DIST30)
    for k in (1, 2, 3):                                 # a 15-bit code (symbols 261 and 262: lengths 7 and 8) exactly at the start of segments 1, 2 and 3
        st._tokens(pad_literals(t0 + SEG * k - st.bitpos, ONE_PREFIX, rng), lc, dc, False)
        assert st.bitpos == t0 + SEG * k and ONE_PREFIX[261 + k % 2] == 15
        st._tokens([match(7 + k % 2, 3)], lc, dc, False)
    st._tokens([], lc, dc, True)
    st.fixed([], final=True)
    assert 8 * len(st.body()) - t0 <= 64 * SEG
    V("longest_code_first_in_a_segment", st, "a 15-bit lit/len code that starts on the first bit of the parallel decoder's segments 1, 2 and 3")
    V("all_286_litlen_symbols_in_use", Stream().dynamic(lits(bytes(range(256))) + [match(LBASE[k], 100 + k) for k in range(29)], FLAT286, DIST30, final=True),
      "every one of the 286 lit/len symbols occurs")
    V("fixed_code_range_edges", Stream().fixed([lit(0), lit(143), lit(144), lit(255), match(3, 2), match(114, 4, lsym=279), match(115, 1, lsym=280), match(258, 3)], final=True),
      "the fixed code's 8-bit (0, 143, 280, 285), 9-bit (144, 255) and 7-bit (256, 257, 279) ranges at their first and last symbols")
    # ---- segments of the parallel decoder
    for k in (1, 2, 63, 64):
        for d in (-1, 0, 1):
            V("segments_span_%d" % (SEG * k + d), seg_stream(SEG * k + d), "%d bits of tokens: %d segments' worth %+d" % (SEG * k + d, k, d))
    rng = _rng("segs")
    st = Stream()
    st.b.put(0, 1); st.b.put(1, 2)
    st._tokens(pad_literals(2 * SEG, FIXED_LL, rng), _codes(FIXED_LL), _codes(FIXED_DL), True)
    assert st.bitpos == 3 + 2 * SEG + 7
    V("end_of_block_first_in_a_segment", st.fixed(lits(_rb(rng, 60)) + [match(9, 70)], final=True), "the end-of-block code on the first bit of segment 2")
    st = Stream().fixed(lits(_rb(rng, 20)))
    p0 = st.bitpos
    st.dynamic(lits(_rb(rng, 150)) + [match(40, 160)], FLAT286, DIST30, mode="plain", cl_weights={k: 1 for k in range(19)}, final=True)
    assert st.tokens_at - p0 > 3 * SEG
    V("dynamic_header_longer_than_a_segment", st, "a second block whose dynamic header is several segments long: the lanes that start inside it walk garbage")
    toks = lits(_rb(rng, 4000))
    for i in range(900):
        toks.append(match(3, 3000 + i % 50) if i % 2 == 0 else match(4, 120 + i % 7))
    V("more_waiting_matches_than_the_list_holds", Stream().fixed(toks, final=True),
      "900 matches in one round whose sources other lanes write (the list holds 768: the round is cut), every other one copying what such matches wrote (a chain)")
    # ---- zlib header
    rng = _rng("hdr")
    far = Stream().fixed(lits(_rb(rng, 32768)) + [match(258, 32768), match(3, 32507), match(258, 32506), match(3, 257), match(258, 32767)], final=True)
    for ci in (0, 7):
        V("cinfo%d_far_distances" % ci, far, "CINFO %d in the header, distances up to 32768 in the data (stock zlib does not hold a stream to its CINFO)" % ci, cinfo=ci)
    for fl in range(4):
        V("flevel%d_far_distances" % fl, far, "FLEVEL %d" % fl, flevel=fl)

    # ---- malformed
    good = Stream().fixed(lits(b"payload") + [match(20, 7)], final=True)
    M("header_cm_7", good.zlib(cm=7), 1, "compression method 7")
    M("header_cinfo_8", good.zlib(cinfo=8), 1, "CINFO 8: a 64 KiB window")
    M("header_bad_fcheck", good.zlib(fcheck=(good.zlib()[1] + 1) & 31), 1, "CMF * 256 + FLG is no multiple of 31")
    M("header_fdict", good.zlib(fdict=1), 1, "FDICT: a preset dictionary")
    M("block_type_3", Stream().raw(1, 1).raw(3, 2).raw(0, 61).zlib(adler=1), 2, "block type 3")
    M("stored_nlen_mismatch", Stream().stored(b"abcdef", final=True, nlen=0xFFF8).zlib(), 2, "NLEN is not the complement of LEN")
    M("stored_len_past_the_end", Stream().stored(b"abcdef", final=True, length=7).zlib(), 3, "a stored block one byte longer than the deflate data")
    for s in (286, 287):
        M("fixed_litlen_symbol_%d" % s, Stream().fixed(lits(b"abc") + [sym(s)], final=True).zlib(), 2, "lit/len symbol %d of the fixed code" % s)
    for s in (30, 31):
        M("fixed_distance_symbol_%d" % s, Stream().fixed(lits(b"abc") + [match(3, 1, dsym=s)], final=True).zlib(), 2, "distance symbol %d of the fixed code" % s)
    for n in (287, 288):
        M("hlit_%d" % n, Stream().dynamic(lits(b"abc"), FLAT286 + [0] * (n - 286), DIST30, final=True).zlib(), 2, "HLIT says %d lit/len codes" % n)
    for n in (31, 32):
        M("hdist_%d" % n, Stream().dynamic(lits(b"abc"), FLAT286, DIST30 + [0] * (n - 30), final=True).zlib(), 2, "HDIST says %d distance codes" % n)
    plain = lits(b"the only fault is the code")
    body = plain + [match(8, 3)]
    M("code_length_code_oversubscribed", Stream().dynamic(plain, FLAT257, [1, 1], mode="plain", cll=_cl({8: 1, 9: 1, 1: 1}), final=True).zlib(), 2, "three 1-bit codes in the code-length code")
    M("code_length_code_incomplete", Stream().dynamic(plain, FLAT257, [1, 1], mode="plain", cll=_cl({8: 2, 9: 2, 1: 2}), final=True).zlib(), 2,
      "three 2-bit codes in the code-length code; every code the sequence uses exists")
    M("litlen_code_oversubscribed", Stream().dynamic(plain + [match(3, 2)], [8] * 258, [1, 1], final=True).zlib(), 2, "258 lit/len codes of 8 bits")
    M("litlen_code_incomplete", Stream().dynamic(plain, [8] * 254 + [0, 0, 8], [1, 1], final=True).zlib(), 2, "255 lit/len codes of 8 bits; every code the block uses exists")
    M("litlen_single_code_of_2_bits", Stream().dynamic([], [0] * 256 + [2], [0], final=True).zlib(), 2, "a lone end-of-block code of 2 bits (only a lone 1-bit code may be incomplete)")
    M("distance_code_oversubscribed", Stream().dynamic(body, FLAT286, [1, 1, 1], final=True).zlib(), 2, "three 1-bit distance codes")
    M("distance_code_incomplete", Stream().dynamic(body, FLAT286, [2, 2, 2], final=True).zlib(), 2, "three 2-bit distance codes; every code the block uses exists")
    M("distance_single_code_of_2_bits", Stream().dynamic(lits(b"abc") + [match(8, 1)], FLAT286, [2], final=True).zlib(), 2, "a lone distance code of 2 bits")
    M("distance_codes_30_of_5_bits", Stream().dynamic(body, FLAT286, [5] * 30, final=True).zlib(), 2, "30 distance codes of 5 bits in a DYNAMIC block: incomplete (the fixed code has 32)")
    M("no_end_of_block_code", Stream().dynamic(lits(b"abc"), [8] * 256 + [0], [1, 1], final=True, eob=False).raw(0, 40).zlib(), 2, "symbol 256 has length 0")
    M("length_symbol_without_distance_code", Stream().dynamic(lits(b"abc") + [sym(257)], [8] * 254 + [9] * 4, [0], final=True).zlib(), 2, "a length symbol in a block that has no distance code")
    M("too_far_first_token", Stream().fixed([match(3, 1)], final=True).zlib(), 2, "a match as the first token of the stream")
    for k in (1, 5, 258, 4097):
        M("too_far_after_%d_literals" % k, Stream().fixed(lits(_rb(_rng("tf%d" % k), k)) + [match(3, k + 1)], final=True).zlib(), 2, "distance %d with %d bytes out" % (k + 1, k))
    M("too_far_behind_stored_block", Stream().stored(_rb(rng, 100)).fixed([match(3, 101)], final=True).zlib(), 2, "distance 101 behind a stored block of 100 bytes")
    M("too_far_32768_with_32767_out", Stream().fixed(lits(_rb(rng, 32767)) + [match(3, 32768)], final=True).zlib(), 2, "distance 32768 with 32767 bytes out")
    M("too_far_in_a_later_window", Stream().fixed(lits(_rb(rng, 6000)) + [match(3, 6001)], final=True).zlib(), 2,
      "distance 6001 with 6000 bytes out, in the second 4 KiB of the stream: not in the parallel decoder's first segment")
    M("bad_adler", good.zlib(adler=(zlib.adler32(bytes(good.out)) ^ 0x10000) & 0xFFFFFFFF), 4, "one bit of the Adler-32 flipped")
    M("byte_between_last_block_and_adler", bytes(good.zlib()[:-4]) + b"\x00" + good.zlib()[-4:], 4, "a byte between the final block and the Adler-32: the trailer is not where the stream says")
    M("bytes_behind_the_adler", good.zlib(tail=b"\x00\x01\x02"), None, "three bytes behind the Adler-32 (outside the referee's judgement: only 'never status 0 with other bytes' is pinned)")
    st = Stream().fixed(lits(b"never ends" + bytes([200] * 6)))
    assert st.bitpos % 8 == 0
    M("no_final_block", st.zlib(), 3, "the only block is not final (it ends on a byte: the next block header is the first thing missing)")
    st, at = _cut_base()
    whole = st.zlib()
    assert py_inflate(whole).data == bytes(st.out)
    for n in (1, 2, 5):
        M("cut_to_%d_bytes" % n, whole[:n], 3, "%d bytes: shorter than header and trailer" % n)
    for place, p in sorted(at.items(), key=lambda kv: kv[1]):
        cut = whole[:p // 8 + 6]
        r = py_inflate(cut, "device")
        assert r.status in (2, 3), (place, r.status)
        M("cut_in_%s" % place, cut, r.status, "the deflate data ends in front of bit %d (%s)%s" % (p, place.replace("_", " "),
          "" if r.status == 3 else ": 2, because the zero bits behind the end are read as '%s' before the end is noticed" % r.reason))
    for k in (1, 2, 3, 4):
        M("cut_%d_bytes_off_the_adler" % k, whole[:-k], 3, "%d bytes short: the last four bytes are taken for the trailer, and the final block has lost its end" % k)
    assert len({e.name for e in E}) == len(E)
    return E


def by_name():
    return {e.name: e for e in catalogue()}
