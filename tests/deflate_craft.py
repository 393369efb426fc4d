"""Hand-made DEFLATE for the inflate tests (test infrastructure; STOCK zlib is the referee of what is valid — RFC 1950 / 1951).

Two layers.  The first (dynamic_block, zlib_stream, raw_stream_with_sequence: the header tests of test_gpu_parity.py) writes one dynamic
block of literals and varies its HEADER:

  lit/len code lengths   chosen by the caller (any complete canonical code)
  sequence tokens        "plain": one token per length, "rle": zlib-like runs, "rep0": symbol 16 behind zero lengths as well
  code-length code       from the token frequencies (Huffman, limited to 7 bits), or from caller's weights (shapes with 1-bit codes)

The second (Stream, py_inflate, catalogue; tests/test_inflate_craft.py) writes whole streams token by token — stored, fixed and dynamic
blocks at any bit offset, any symbol and extra-bit choice, any code lengths, complete or not, any zlib wrapper — executes its own tokens to
know what a valid stream holds, and restates inflate in plain Python from the RFCs, with zlib's rules for the code tables.

A third part, for the ENCODER (tests/test_deflate_encode_craft.py), stands at the end: parse_blocks reads a stream down to header fields,
code-length entries and tokens; rle_tokens, cl_rle and the cost functions restate the encoder's rules; encode_catalogue names record
payloads that reach its edges.
"""
import collections
import functools
import heapq
import re
import struct
import types
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


# ================================================================ the ENCODER's side: what a record's stream holds, token by token
# (tests/test_deflate_encode_craft.py).  parse_blocks reads a zlib stream down to its header fields, code-length entries and tokens;
# rle_tokens, cl_rle and the cost functions restate what csrc/deflate2_dev.h and cl_header_wave (csrc/deflate_dev.h) promise in their
# comments — the rule, in plain Python over bytes and lists, not the kernels' mask arithmetic —; encode_catalogue names the smallest
# record payloads that reach each edge of the encoder.
BLOCK = 16384                    # DEFL_BLK: payload bytes of one DEFLATE block (the staged form cuts there; the fused kernels take one block)
SLAB = 256                       # positions of a wave step: slab k covers [256 k - 2, 256 k + 254), a lane four of them
DEFL2_LIST_CAP = 640             # tokens of the list in S.freq
DEFL2_LISTB_MIN = 64             # the list's second pool (staged form) never reaches below this word of the bit buffer
STAGED_OBUF_WORDS = (BLOCK + 64) // 4          # staged_shape(): words of the staged kernel's bit buffer
STAGED_WF_AT = STAGED_OBUF_WORDS - 4 * 288     # ... below its four per-wave histograms: the second pool grows down from here
LIST_CAP_STAGED = DEFL2_LIST_CAP + (STAGED_WF_AT - DEFL2_LISTB_MIN) * 2
# the two static code-length codes of cl_header_wave, as data: lengths of symbols 0 .. 18
CLA_LENS = [3, 7, 7, 7, 7, 5, 5, 5, 5, 5, 3, 2, 2, 7, 0, 0, 5, 6, 7]      # HCLEN 18 (symbol 15 stands last in ORDER and has no code)
CLB_LENS = [3, 6, 7, 7, 6, 5, 4, 5, 5, 4, 3, 3, 2, 7, 7, 7, 4, 6, 7]      # HCLEN 19
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def _peek_table(lengths):
    """([(symbol, length) or None] indexed by the next m bits of the stream, m = the longest length) of a canonical code"""
    m = max(lengths) if lengths else 0
    tab = [None] * (1 << m)
    for s, (c, l) in enumerate(zip(canonical(list(lengths)), lengths)):
        if l:
            r = int(format(c, "0%db" % l)[::-1], 2)
            for k in range(r, 1 << m, 1 << l):
                tab[k] = (s, l)
    return tab, m


@functools.lru_cache(maxsize=None)          # (the routes hand in the same streams again and again; the result is read, never changed)
def parse_blocks(stream):
    """RFC 1950 / 1951 on `stream`, keeping what py_inflate throws away.  -> namespace(header, blocks, data, adler, trailing); a block:
    btype, bfinal, first_bit, end_bit (bit positions in the deflate data: the block is [first_bit, end_bit)), at (bytes out in front of
    it), data (the bytes it produces); stored: pad (the bits up to the byte boundary); Huffman: tokens [("L", byte) | ("M", length,
    distance)], tokens_at; dynamic: hlit, hdist, hclen, cll (the 19 code-length-code lengths), entries [(symbol, extra value)] of the
    code-length sequence as sent, litlens, dlens.  adler: the four bytes behind the last block as a number, trailing: what follows them.
    ValueError on anything that is not a stream."""
    if len(stream) < 6 or (stream[0] & 15) != 8 or (stream[0] >> 4) > 7 or (stream[0] * 256 + stream[1]) % 31 or stream[1] & 0x20:
        raise ValueError("zlib header")
    d = stream[2:]
    nbits = 8 * len(d)

    def peek(pos, n):                          # n <= 25
        return (int.from_bytes(d[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)

    pos, out, blocks = 0, bytearray(), []
    while True:
        b = types.SimpleNamespace(first_bit=pos, at=len(out))
        b.bfinal, b.btype = peek(pos, 1), peek(pos + 1, 2)
        pos += 3
        if b.btype == 3:
            raise ValueError("block type 3")
        if b.btype == 0:
            padn = -pos & 7
            b.pad = peek(pos, padn)
            pos += padn
            ln, nl = peek(pos, 16), peek(pos + 16, 16)
            pos += 32
            if ln ^ nl != 0xFFFF or (pos >> 3) + ln > len(d):
                raise ValueError("stored block")
            out += d[pos >> 3:(pos >> 3) + ln]
            pos += 8 * ln
        else:
            if b.btype == 1:
                ll, dl = FIXED_LL, FIXED_DL
            else:
                b.hlit, b.hdist, b.hclen = peek(pos, 5) + 257, peek(pos + 5, 5) + 1, peek(pos + 10, 4) + 4
                pos += 14
                if b.hlit > 286 or b.hdist > 30:
                    raise ValueError("HLIT / HDIST")
                b.cll = [0] * 19
                for k in range(b.hclen):
                    b.cll[ORDER[k]] = peek(pos, 3)
                    pos += 3
                if sum(1 << (7 - l) for l in b.cll if l) != 128:
                    raise ValueError("code-length code")
                ct, cm = _peek_table(b.cll)
                b.entries, lens = [], []
                while len(lens) < b.hlit + b.hdist:
                    s, l = ct[peek(pos, cm)]
                    pos += l
                    x = peek(pos, CL_EXTRA.get(s, 0))
                    pos += CL_EXTRA.get(s, 0)
                    if s == 16 and not lens:
                        raise ValueError("repeat with nothing in front")
                    lens += [s] if s < 16 else [lens[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
                    b.entries.append((s, x))
                if len(lens) > b.hlit + b.hdist or pos > nbits:
                    raise ValueError("code-length sequence")
                ll, dl = b.litlens, b.dlens = lens[:b.hlit], lens[b.hlit:]
            lt, lm = _peek_table(ll)
            dt, dm = _peek_table(dl)
            b.tokens_at, b.tokens = pos, []
            while True:
                e = lt[peek(pos, lm)]
                if e is None or pos > nbits:
                    raise ValueError("lit/len code")
                pos += e[1]
                s = e[0]
                if s < 256:
                    b.tokens.append(("L", s))
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise ValueError("lit/len symbol %d" % s)
                    length = LBASE[s - 257] + peek(pos, LEXT[s - 257])
                    pos += LEXT[s - 257]
                    e = dt[peek(pos, dm)] if dm else None
                    if e is None or e[0] >= 30:
                        raise ValueError("distance code")
                    pos += e[1]
                    dist = DBASE[e[0]] + peek(pos, DEXT[e[0]])
                    pos += DEXT[e[0]]
                    if dist > len(out):
                        raise ValueError("distance %d with %d bytes out" % (dist, len(out)))
                    b.tokens.append(("M", length, dist))
                    if dist >= length:
                        out += out[len(out) - dist:len(out) - dist + length]
                    else:
                        for _ in range(length):
                            out.append(out[-dist])
        if pos > nbits:
            raise ValueError("truncated")
        b.end_bit, b.data = pos, bytes(out[b.at:])
        blocks.append(b)
        if b.bfinal:
            break
    end = (pos + 7) >> 3
    if len(d) < end + 4:
        raise ValueError("truncated")
    return types.SimpleNamespace(header=bytes(stream[:2]), blocks=blocks, data=bytes(out), adler=struct.unpack(">I", d[end:end + 4])[0], trailing=bytes(d[end + 4:]))


def as_stream_tokens(tokens):
    """parse_blocks' tokens as Stream's"""
    return [lit(t[1]) if t[0] == "L" else match(t[1], t[2]) for t in tokens]


def emit_blocks(p):
    """the stream that parse_blocks read, written again from what it returned: canonical codes from the lengths, the code-length
    entries as sent, every token with the one symbol and extra-bit choice an encoder makes"""
    w = Bits()
    for b in p.blocks:
        w.put(b.bfinal, 1)
        w.put(b.btype, 2)
        if b.btype == 0:
            if w.n:
                w.put(b.pad, 8 - w.n)
            w.put(len(b.data), 16)
            w.put(len(b.data) ^ 0xFFFF, 16)
            w.out += b.data
            continue
        ll, dl = FIXED_LL, FIXED_DL
        if b.btype == 2:
            ll, dl = b.litlens, b.dlens
            w.put(b.hlit - 257, 5); w.put(b.hdist - 1, 5); w.put(b.hclen - 4, 4)
            for k in range(b.hclen):
                w.put(b.cll[ORDER[k]], 3)
            cc = _codes(b.cll)
            for s, x in b.entries:
                w.put(*cc[s])
                w.put(x, CL_EXTRA.get(s, 0))
        lc, dc = _codes(ll), _codes(dl)
        for t in as_stream_tokens(b.tokens):
            if t[0] == "lit":
                w.put(*lc[t[1]])
            else:
                w.put(*lc[t[3]]); w.put(t[4], LEXT[t[3] - 257]); w.put(*dc[t[5]]); w.put(t[6], DEXT[t[5]])
        w.put(*lc[256])
    return p.header + w.done() + struct.pack(">I", p.adler) + p.trailing


# ---------------------------------------------------------------- the tokeniser, restated from the head comment of csrc/deflate2_dev.h
def runs_of(data):
    """[(first position, length)] of the maximal runs of equal bytes"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if not len(a):
        return []
    starts = np.concatenate([[0], np.flatnonzero(a[1:] != a[:-1]) + 1])
    return list(zip(starts.tolist(), np.diff(np.concatenate([starts, [len(a)]])).tolist()))


def rle_tokens(block_bytes):
    """the tokens of ONE block: a run of R <= 3 equal bytes is R literals; a run of R >= 4 is one literal, (R - 1) // 258 matches
    (258, distance 1), and for rem = (R - 1) % 258 one match (rem, 1) if rem >= 3, else rem literals"""
    out = []
    for s, r in runs_of(block_bytes):
        v = block_bytes[s]
        if r <= 3:
            out += [("L", v)] * r
            continue
        out.append(("L", v))
        out += [("M", 258, 1)] * ((r - 1) // 258)
        rem = (r - 1) % 258
        out += [("M", rem, 1)] if rem >= 3 else [("L", v)] * rem
    return out


def pieces(payload):
    """the blocks of a payload: the staged form cuts at every 16384 bytes (a payload of at most one block is one block; an empty one too)"""
    return [payload[i:i + BLOCK] for i in range(0, len(payload), BLOCK)] or [b""]


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "L":
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


def slab_token_counts(block_bytes):
    """{slab: tokens} of the GENERAL slabs of a block, the ones whose tokens pass 1 puts on the list: slab k covers positions
    [256 k - 2, 256 k + 254); it is general if one of its positions lies in a run of >= 4 bytes behind that run's first byte.  A literal
    counts at its own position, what a run sends behind its first byte at the run's LAST position."""
    general, count = set(), collections.Counter()
    for s, r in runs_of(block_bytes):
        if r <= 3:
            for p in range(s, s + r):
                count[(p + 2) // SLAB] += 1
            continue
        count[(s + 2) // SLAB] += 1
        rem = (r - 1) % 258
        count[(s + r - 1 + 2) // SLAB] += (r - 1) // 258 + (1 if rem >= 3 else rem)
        general.update(range((s + 1 + 2) // SLAB, (s + r - 1 + 2) // SLAB + 1))
    return {k: count[k] for k in sorted(general)}


# ---------------------------------------------------------------- costs, from a token list: exact integer arithmetic
def token_symbol(t):
    """(lit/len symbol, extra bits) of a token"""
    if t[0] == "L":
        return t[1], 0
    k = 28 if t[1] == 258 else max(s for s in range(28) if LBASE[s] <= t[1])
    return 257 + k, LEXT[k]


def _dist_symbol(dist):
    return max(s for s in range(30) if DBASE[s] <= dist)


def token_freq(tokens):
    """occurrences of the 286 lit/len symbols, the end-of-block code counted once"""
    f = [0] * 286
    for t in tokens:
        f[token_symbol(t)[0]] += 1
    f[256] += 1
    return f


def _side_bits(tokens, fixed):
    """length extra bits + what the distances take: 5 bits + extra under the fixed code, 1 bit under the encoder's two 1-bit codes"""
    n = 0
    for t in tokens:
        if t[0] == "M":
            n += token_symbol(t)[1] + (5 + DEXT[_dist_symbol(t[2])] if fixed else 1)
    return n


def fixed_bits(tokens):
    """a fixed block: 3 + body under the fixed code + 7"""
    return 3 + sum(FIXED_LL[token_symbol(t)[0]] for t in tokens) + _side_bits(tokens, True) + 7


def stored_bits(at_bit, n):
    """a stored block of n bytes whose header starts at bit at_bit: 3 + pad to the byte + 32 + 8 n"""
    return 3 + (-(at_bit + 3) & 7) + 32 + 8 * n


def shannon_lengths(freq):
    """ceil(log2(N / f)) per symbol in use, N = sum(freq): the smallest l with f << l >= N (where assign_lengths_wave starts; <= 15 for
    N <= 32768)"""
    N = sum(freq)
    return [0 if not f else next(l for l in range(1, 32) if (f << l) >= N) for f in freq]


def shannon_body_bits(tokens):
    """sum over the tokens' symbols of f * ceil(log2(N / f)), N = tokens + one end-of-block, + the matches' extra and distance bits (the
    end-of-block code itself is not in it)"""
    f = token_freq(tokens)
    ls = shannon_lengths(f)
    f[256] -= 1
    return sum(a * b for a, b in zip(f, ls)) + _side_bits(tokens, False)


def dyn_upper(tokens, hlit=286):
    """what the encoder's own dynamic block costs at most: 17 header bits, 19 code-length-code lengths, <= 7 bits per code length
    described (an entry of either static code-length code costs at most that per length it covers), the body at its Shannon start
    (assign_lengths_wave only shortens the codes of symbols in use), an end-of-block code of <= 15 bits"""
    return 17 + 3 * 19 + 7 * (hlit + 2) + shannon_body_bits(tokens) + 15


def huffman_body_bits(tokens):
    """the body under an optimal Huffman code of the tokens' symbols and end-of-block (no dynamic block has a smaller body; nor has the
    fixed one), the matches' extra and distance bits as the encoder's dynamic block sends them"""
    f = token_freq(tokens)
    ls = huff_lengths(f, 15) if sum(1 for x in f if x) >= 2 else [1 if x else 0 for x in f]
    return sum(a * b for a, b in zip(f, ls)) + _side_bits(tokens, False)


def dyn_lower(tokens):
    """what ANY dynamic block of this encoder costs at least: 17 header bits, 18 code-length-code lengths (either static code sends 18
    or 19), one bit per symbol that needs a code (the cheapest description of a nonzero length is a share of a symbol-16 entry: 4 + 2
    bits for six of them), and the body under an optimal Huffman code, end-of-block included"""
    return 17 + 3 * 18 + sum(1 for f in token_freq(tokens) if f) + huffman_body_bits(tokens)


def pinned_type(tokens, n):
    """the block type that the arithmetic alone pins for a block of n bytes, wherever its header starts in a byte: 2 if the dynamic
    block's upper bound beats the fixed block and the shortest stored one (the encoder takes the dynamic block unless one of the others
    is no larger); 0 if the longest stored block is no larger than the fixed block and than dyn_lower (stored wins ties); else None"""
    if dyn_upper(tokens) < min(fixed_bits(tokens), stored_bits(5, n)):
        return 2
    if stored_bits(6, n) <= min(fixed_bits(tokens), dyn_lower(tokens)):
        return 0
    return None


def cl_rle(lengths):
    """the header's run-length rule as [(symbol, extra value)]: zeros in chunks of 138 — a chunk of >= 11 one symbol-18 entry, of 3 .. 10
    one symbol-17 entry, a shorter one plain zeros; of a run of a nonzero value the first goes plain and the rest in chunks of 6 — a chunk
    of >= 3 one symbol-16 entry, a shorter one plain"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        j = i
        while j < n and lengths[j] == lengths[i]:
            j += 1
        v, run = lengths[i], j - i
        if v == 0:
            for c in [138] * (run // 138) + [run % 138]:
                out += [(18, c - 11)] if c >= 11 else [(17, c - 3)] if c >= 3 else [(0, 0)] * c
        else:
            out.append((v, 0))
            for c in [6] * ((run - 1) // 6) + [(run - 1) % 6]:
                out += [(16, c - 3)] if c >= 3 else [(v, 0)] * c
        i = j
    return out


def cl_cost(entries, cl_lens):
    """bits of the code-length sequence under one of the static codes; None if it lacks a symbol"""
    if any(cl_lens[s] == 0 for s, _ in entries):
        return None
    return sum(cl_lens[s] + CL_EXTRA.get(s, 0) for s, _ in entries)


# ================================================================ the encoder's catalogue: the smallest payload per edge
# A record's payload is [u16 id length][read id][u32 read group][4 doubles][u64 blob length][signal blob][aux bytes]; the aux bytes are
# copied verbatim, so everything behind the head is the test's to choose.  An entry is a dict: name, signal, read_id, fields (read group
# and the four doubles), aux, why; and what the CPU test holds it to — runs [(last position, length)] of the payload, pin (the block type
# per block that the arithmetic must pin, or None), plus per-family keys named where they are made.
SIG4 = (3, 4, 5, 4)                                  # four samples: blob 04 00 00 00 | 00 | 06 02 02 01
FIELDS2 = (0, 2.0, 2.0, 2.0, 2.0)                   # 2.0 = 00 00 00 00 00 00 00 40: small bytes only
ALPHA16 = bytes(range(0x61, 0x71))                  # the background's 16 values
RUN_BYTES = bytes(range(0xE0, 0xF0))                # planted runs: outside the background, neighbours differ


def enc_hdr(e):
    """the record bytes in front of the u64 blob length (press.pack_hdr)"""
    return struct.pack("<H", len(e["read_id"])) + e["read_id"] + struct.pack("<Idddd", *e["fields"])


def enc_payload(e, sig_method=1):
    """the oracle's payload of an entry (sig_method 1 svb-zd, 2 ex-zd)"""
    key = (e["name"], sig_method)
    if key not in _PAYLOADS:
        import oracle_bind as ob
        r, keep = ob.make_rec(e["read_id"], *e["fields"], np.asarray(e["signal"], dtype=np.int16), e["aux"])
        _PAYLOADS[key] = ob.rec_pack(r, sig_method)
    return _PAYLOADS[key]


_PAYLOADS = {}


def background(rng, n, alphabet=ALPHA16):
    """n bytes over the alphabet with no run of four"""
    x = rng.integers(0, len(alphabet), n)
    for i in range(3, n):
        if x[i] == x[i - 1] == x[i - 2] == x[i - 3]:
            x[i] = (x[i] + 1) % len(alphabet)
    return bytearray(bytes(alphabet[int(v)] for v in x))


def flat_bytes(rng, n):
    """n bytes (a multiple of 256), every value equally often, in a shuffled order without a run of four"""
    while True:
        x = bytes(rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), n // 256)))
        if all(r < 4 for _, r in runs_of(x)):
            return bytearray(x)


@functools.lru_cache(maxsize=None)
def encode_catalogue():
    """[entry dict] (needs the CPU oracle: the head of every payload is the oracle's)"""
    E = []

    def head_of(signal, read_id, fields):
        e = dict(name="head:%r%r%r" % (tuple(signal), read_id, fields), signal=signal, read_id=read_id, fields=fields, aux=b"")
        return enc_payload(e)

    def add(name, why, plen=None, runs=(), aux=None, signal=SIG4, read_id=b"craft0001", fields=FIELDS2, pin=2, bg=None, **more):
        """plen and runs are in PAYLOAD positions: the aux bytes are a background of plen - head bytes with the runs (last position,
        length) planted in it, run i of byte RUN_BYTES[i % 16]; or aux as given"""
        head = head_of(tuple(signal), read_id, fields)
        if aux is None:
            rng = _rng(name)
            pay = bytearray(head) + (background(rng, plen - len(head)) if bg is None else bg(rng, plen - len(head)))
            for i, (end, r) in enumerate(runs):
                assert end - r + 1 >= len(head) and end < plen, (name, end, r)
                pay[end - r + 1:end + 1] = bytes([RUN_BYTES[i % 16]]) * r
            aux = bytes(pay[len(head):])
        e = dict(name=name, why=why, signal=tuple(signal), read_id=read_id, fields=fields, aux=bytes(aux), runs=list(runs), pin=pin, head=len(head))
        e.update(more)
        E.append(e)
        return e

    P9 = 2250                                            # nine slabs, the last one partly filled: positions up to 2249 of [2046, 2302)
    # ---- runs against the frame geometry
    for off in range(-2, 6):
        where = "slot %d of lane 63 in front of it" % (off + 4) if off < 0 else "slot %d of lane %d" % (off % 4, off // 4)
        for back in (3, 4, 5):
            add("slab_end%+d_back%d" % (off, back), "at every slab boundary 256 k - 2, k = 1 .. 8, a run of %d that ends %+d from it (%s)" % (back + 1, off, where),
                P9, [(SLAB * k - 2 + off, back + 1) for k in range(1, 9)])
        for par, ks in (("odd", (1, 3, 5, 7)), ("even", (2, 4, 6, 8))):
            add("slab_end%+d_back260_%s" % (off, par), "a run that starts in front of the slab it ends in (find_break_before), ending %+d from the boundary of slab %s: 261 "
                "bytes (slab 1: 150, it cannot start in the head)" % (off, ", ".join(map(str, ks))), P9, [(SLAB * k - 2 + off, 261 if k > 1 else 150) for k in ks])
    # (the entries above hold a run in every slab: more tokens of general slabs than the list takes, so WHICH of their slabs are sent from the list
    # and which are redone from the bytes depends on the order in which the waves ask.  These hold one such run, and a run of 180 that
    # leaves slab 0 some 40 tokens: at most 43 + 254 + 254 listed tokens, all of them in S.freq on every route)
    for k in range(1, 9):
        for off in range(-2, 6):
            add("alone_slab%d_end%+d" % (k, off), "a run of 5 that ends %+d from the boundary of slab %d and no other but one in slab 0: every general slab is sent from the list" %
                (off, k), P9, [(243, 180), (SLAB * k - 2 + off, 5)], listed=True)
    P9L = 2300                                           # the last slab filled up to slot 1 of lane 63
    for lane, slab in ((62, 0), (63, 0), (0, 8), (1, 8), (62, 8), (63, 8)):
        for slot in range(4):
            end = SLAB * slab - 2 + 4 * lane + slot
            if end >= P9L:
                continue
            for back in (3, 4, 5):
                add("lane%d_slot%d_slab%d_back%d" % (lane, slot, slab, back), "a run of %d that ends in slot %d of lane %d of %s" %
                    (back + 1, slot, lane, "slab 0" if slab == 0 else "the last, partly filled slab (payload of %d bytes)" % P9L), P9L, [(end, back + 1)])
    add("lane1_slot3_slab0", "a run of 4 in positions 2 .. 5 (the read id): lane 1 of slab 0, whose lane 0 holds positions -2 .. 1", P9, [], read_id=b"AAAAcraft")["runs"] = [(5, 4)]
    for j in (2, 3, 4):
        add("from_position_0_to_%d" % (j + 1), "a run from position 0: an id length of 257 = 01 01 and a read id that starts with %d bytes 01 (slot %d of lane %d of slab 0)" %
            (j, (j + 3) % 4, (j + 3) // 4), 2600, [], read_id=b"\x01" * j + b"craftcraf" * 28 + b"cra"[:257 - j - 252])["runs"] = [(j + 1, j + 2)]
    add("from_position_0_whole_id", "a run of 263 from position 0: id length 01 01, 257 id bytes 01, read group 01 01 01 01", 2600, [], read_id=b"\x01" * 257,
        fields=(0x01010101, 2.0, 2.0, 2.0, 2.0))["runs"] = [(262, 263)]
    for plen in (2250, 2251, 2252, 2253, 2301, 2302, 2303, 2304, 2305, 2306):
        add("length_%d" % plen, "a payload of %d bytes (%d mod 4, %d mod 256), no run at its end" % (plen, plen % 4, plen % 256), plen, [(1200, 5)])
        add("length_%d_run_to_the_end" % plen, "a payload of %d bytes (%d mod 4, %d mod 256) that ends with a run of 5" % (plen, plen % 4, plen % 256), plen, [(plen - 1, 5)])
    add("run_261_to_the_end", "a run that starts two slabs in front of the payload's last byte", P9, [(P9 - 1, 261)])
    # ---- run lengths
    rl = (3, 4, 5, 6, 259, 260, 261, 262, 517, 518, 519, 520)
    at, runs = 100, []
    for r in rl:
        runs.append((at + r - 1, r))
        at += r + 37
    add("run_lengths_around_258", "runs of %s bytes: rem = (R - 1) mod 258 of 0, 1, 2 and 3 behind no, one and two matches of 258" % ", ".join(map(str, rl)), at + 50, runs, rl=rl, pin=None)
    at, runs = 100, []
    for k in range(29):
        runs.append((at + LBASE[k], LBASE[k] + 1))
        at += LBASE[k] + 1 + 23
    add("length_symbols_all_29", "one run of base length + 1 per length symbol 257 .. 285", at + 50, runs, pin=None)
    add("run_16000", "one run of 16000 bytes: 62 matches of 258 from one lane (nfull = 62) and a match of 3", 16200, [(16100, 16000)], pin=None)
    # ---- the run-heavy front (gen_hint): four samples above; here a constant signal of 2000 samples = 499 zero key bytes + 1999 zero data bytes
    const = (1234,) * 2000
    h2 = len(head_of(const, b"craft0001", FIELDS2))
    k2 = (h2 + 2) // SLAB + 2                            # a slab well inside the aux bytes, behind the hinted front
    add("const2000_plain_aux", "constant signal: 499 zero key bytes and 1999 zero data bytes, the first 3 slabs hinted as run-heavy; aux without a run: plain slabs taken in pairs", h2 + 2300, [], signal=const)
    add("const2000_run_in_a_plain_pair", "... and one run of 5 in the second slab of a pair that pass 1 takes for plain", h2 + 2300, [(SLAB * (k2 + 1) + 100, 5)], signal=const)
    add("const2000_runs_at_slab_edges", "... and a run of 5 ending on the first slot of every slab behind the front", h2 + 2300,
        [(SLAB * k - 2, 5) for k in range(k2, (h2 + 2300) // SLAB)], signal=const)
    add("const2000_run_from_the_front", "... whose zero run of the signal continues 300 bytes into the aux bytes", h2 + 2300, [], signal=const,
        aux=b"\x00" * 300 + bytes(background(_rng("c2f"), 2000)))
    # ---- the token list
    for name, plen in (("list_8k_run_in_every_slab", 8192), ("list_16k_run_in_every_slab", BLOCK)):
        add(name, "%d bytes, a run of 4 in every slab: ~254 tokens per general slab, DEFL2_LIST_CAP = %d is full after two or three slabs — fused: the rest take SEG_REDO; staged: "
            "the list straddles entry %d into pool B%s" % (plen, DEFL2_LIST_CAP, DEFL2_LIST_CAP,
            ", fills its %d entries (%d + 2 x (wf_at %d - DEFL2_LISTB_MIN %d)) and leaves the block's ~8 KiB of bits %d words: !list_ok" %
            (LIST_CAP_STAGED, DEFL2_LIST_CAP, STAGED_WF_AT, DEFL2_LISTB_MIN, DEFL2_LISTB_MIN) if plen == BLOCK else ""),
            plen, [(SLAB * k + 130, 4) for k in range(plen // SLAB)], list_over=LIST_CAP_STAGED if plen == BLOCK else DEFL2_LIST_CAP)
    add("poolb_list_ok_dynamic", "16384 bytes, a run of 4 in slabs 0 .. 5 only: ~1500 listed tokens straddle entry %d and take ~%d words of pool B below word %d; the block's bits "
        "(58 plain slabs of 4-bit literals: ~2100 words) end below them: list_ok, and the block stays dynamic" % (DEFL2_LIST_CAP, (1500 - DEFL2_LIST_CAP) // 2, STAGED_WF_AT),
        BLOCK, [(SLAB * k + 130, 4) for k in range(6)], list_over=DEFL2_LIST_CAP, list_ok=True)
    # ---- code lengths and header
    def two_and_rares(rng, n):
        x = bytearray(b"\x61\x62" * (n // 2 + 1))[:n]
        for i in range(n // 250):
            x[100 + 250 * i] = 0x80 + i % 60
        return x
    add("cl14_two_bytes_and_rares", "16384 bytes, two bytes alternating and 60 bytes that occur once or twice: the head's zero runs leave N just below 2^14, the Shannon start holds "
        "lengths of 14, which code-length code A cannot describe", BLOCK, [], bg=two_and_rares)
    add("cl15_later_block", "the same in two blocks: the second has no run at all, N = 16385 > 2^14 and a Shannon start with lengths of 15 (staged form only)", 2 * BLOCK, [],
        bg=two_and_rares)
    at, runs = 400, []
    for k in range(29):
        runs.append((at + LBASE[k], LBASE[k] + 1))
        at += LBASE[k] + 1 + 9
    add("all_286_symbols", "every literal 0 .. 255 and every length symbol in use: no unused symbol is left to absorb the slack", at + 600, runs,
        bg=lambda rng, n: bytearray(bytes(range(256)) * (n // 256 + 1))[:n], all_symbols=True, pin=None)
    # used symbols of these: 0 (the head's zeros), 0x20 .. 0x2F (every other head byte: id length 32, id, read group, doubles, 32 samples with deltas +16 / -17), 256, and the
    # length symbols of the head's zero runs; symbols 1 .. 31 stay unused BELOW the gaps of interest: the slack absorption takes the lowest unused symbols, at most 15 of them
    zsig = tuple(int(v) for v in np.cumsum(np.tile([16, -17], 16)))
    zfields = (0x20212223, ) + tuple(struct.unpack("<d", bytes([0x28 + i, 0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0x27]))[0] for i in range(4))
    for gaps in ((2, 10, 138), (3, 11, 139), (140,)):
        used, s = list(range(0x20, 0x30)), 0x30
        for g in gaps:
            s += g
            used.append(s)
            s += 1
        used += list(range(s, 256))
        add("zero_runs_" + "_".join(map(str, gaps)), "lit/len symbols in use: 0, 0x20 .. 0x2F, then gaps of exactly %s unused symbols (above symbols 1 .. 31, which the slack "
            "absorption may take), then everything up to 255" % ", ".join(map(str, gaps)), 1800, [], signal=zsig, read_id=b"\x21" * 32, fields=zfields,
            bg=lambda rng, n, used=used: background(rng, n, bytes(used)), zero_runs=gaps)
    for rep in (4, 7, 8, 10):
        alpha = bytes(range(0x80, 0x80 + rep))
        add("cl_repeat_%d" % rep, "%d neighbouring symbols 0x80 .. of one frequency between unused ones: a run of %d equal code lengths" % (rep, rep), 64 + 40 * rep, [],
            bg=lambda rng, n, alpha=alpha: bytearray((alpha * (n // len(alpha) + 1))[:n // len(alpha) * len(alpha)] + b"\x7e" * (n % len(alpha))), pin=None, repeat=rep)
    add("hlit_286_only_match_258", "a run of 259: the only match behind the head's is one of 258, symbol 285, HLIT = 286", 900, [(700, 259)], pin=None)
    add("no_match_behind_the_head", "no run of four behind the head (its u64 blob length always holds one: no record's first block has HLIT = 257)", 900, [])
    # ---- block choice
    add("shortest_record", "the shortest payload a record can have: empty signal, one-character read id, no aux (51 bytes)", aux=b"", signal=(), read_id=b"r", pin=None)
    for plen in (100, 300):
        add("payload_%d" % plen, "a payload of %d bytes" % plen, plen, [], pin=None)
    rnd = lambda rng, n: bytearray(_rb(rng, n))
    add("random_with_three_runs", "8100 random bytes with three planted runs: stored (a random payload of a few KB has an optimal Huffman body well below 8 bits per byte: only from "
        "~8 KB on does the arithmetic pin the stored block)", 8100, [(400, 5), (4800, 4), (7300, 6)], bg=rnd, pin=0)
    add("random_1500_with_three_runs", "1500 random bytes with three planted runs", 1500, [(400, 5), (800, 4), (1300, 6)], bg=rnd, pin=None)
    add("half_random_half_constant", "1000 random bytes, then 1000 equal ones", 2064, [(2063, 1000)], bg=rnd, pin=None)
    # a stored block that the fixed block misses by less than its length extra bits.  A shuffled cycle of all 256 values keeps a dynamic block at
    # 8 bits per literal plus its header; zero doubles in the head (a run of up to 35 zeros: a match with 3 extra bits) and a run or two save
    # the fixed block a few hundred bits, every literal of 144 and more costs it one; high literals are added until the fixed block is half
    # its matches' extra bits larger than the stored one.  (That the dynamic block is larger than both rests on its header of some 500 bits:
    # the arithmetic of the restatement does not pin it.  Three cycles and one run of 12 is the shape at which dyn_lower comes closest to the
    # stored block; with four cycles and a run of 20 the encoder's dynamic block already wins.  So the entry's stored block is an OBSERVED pin,
    # key `observed`: the GPU tests assert it on the svb-zd routes, and if a change to the length assignment ever makes the dynamic block win
    # there, they say that this entry no longer does its job.)
    def near_fixed(name, fields, cycles, nruns, r):
        rng = _rng(name)
        head = head_of(SIG4, b"craft0001", fields)
        pay = bytearray(head)
        for i in range(nruns):
            pay += bytes(rng.permutation(256).astype(np.uint8)[:24]) + bytes([RUN_BYTES[i % 16]]) * r
        for _ in range(cycles):
            pay += flat_bytes(rng, 256)
        toks = rle_tokens(bytes(pay))
        extra = sum(token_symbol(t)[1] for t in toks)
        more = extra // 2 - (fixed_bits(toks) - stored_bits(0, len(pay)))
        assert 0 <= more <= 112, (name, more)
        pay += bytes([144 + (7 * i) % 112 for i in range(more)])
        add(name, "%d bytes of every byte value about equally often, zero doubles in the head and %d run(s) of %d: the fixed block is %d bits larger than the stored one and holds %d "
            "length extra bits; left out of its cost they make it look smaller" % (len(pay), nruns, r, extra // 2, extra), aux=bytes(pay[len(head):]), fields=fields, pin=None, near_fixed=extra, observed=0)
    near_fixed("fixed_near_stored", (0, 0.0, 0.0, 0.0, 0.0), 3, 1, 12)
    # small payloads over alphabets of 3 .. 42 values with skewed frequencies: code-length headers of many shapes (the choice between the two static
    # code-length codes is checked on every one; among so many, some cost the same under both)
    def skewed(k):
        def make(rng, n):
            alpha = rng.permutation(256)[:3 + k]
            p = 0.85 ** np.arange(3 + k)
            x = rng.choice(3 + k, n, p=p / p.sum())
            for i in range(3, n):
                if x[i] == x[i - 1] == x[i - 2] == x[i - 3]:
                    x[i] = (x[i] + 1) % (3 + k)
            return bytearray(bytes(int(alpha[v]) for v in x))
        return make
    for k in range(40):
        add("skewed_%02d" % k, "%d bytes over %d values of geometric frequencies" % (500 + 60 * k, 3 + k), 500 + 60 * k, [], bg=skewed(k), pin=None)
    # ---- block edges (staged form: more than one block)
    for plen in (16383, 16384, 16385, 16386, 16387, 32768, 32769):
        add("payload_%d" % plen, "a payload of %d bytes: blocks of %s" % (plen, " + ".join(str(len(x)) for x in pieces(bytes(plen)))), plen, [(5000, 5)], pin=None)
    add("run_3_before_to_3_behind_the_cut", "a run of 6 across the cut at 16384: three literals at the end of one block, three at the start of the next", 17000, [(BLOCK + 2, 6)])
    add("run_600_across_the_cut", "a run of 600 across the cut at 16384: 300 bytes in either block, starting anew behind the cut", 19500, [(BLOCK + 299, 600)])
    add("stored_then_dynamic", "16384 random bytes, then 3000 compressible ones: the dynamic block's carry word and bit offset come from a stored block", BLOCK + 3000, [],
        bg=lambda rng, n: bytearray(_rb(rng, n - 3000)) + background(rng, 3000), pin=(0, 2))
    add("dynamic_then_stored", "16384 compressible bytes, then every byte value 64 times in a shuffled order: the stored block's pad bits depend on the dynamic block in front; "
        "the second block's optimal Huffman BODY alone is larger than the stored block", 2 * BLOCK, [],
        bg=lambda rng, n: background(rng, n - BLOCK) + flat_bytes(rng, BLOCK), pin=(2, 0), flat_block=1)
    assert len({e["name"] for e in E}) == len(E)
    return E


def enc_family(name):
    """the name with its numbers taken out: the entries of one loop of the catalogue"""
    return re.sub(r"[+-]?\d+", "#", name)


def enc_by_name():
    return {e["name"]: e for e in encode_catalogue()}
