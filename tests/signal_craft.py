"""svb-zd and ex-zd blobs written field by field, their plain references, and the inverse: the signal that must encode to given fields.

Test infrastructure only, in the manner of deflate_craft.py and zstd_craft.py.  Two layers:

  * builders and references (no encoder, no GPU): svb_blob / svb_ref_decode for svb-zd, svb32 / exzd_blob / exzd_ref_decode / fields for
    ex-zd.  tests/test_svbzd_decode.py and tests/test_exzd_decode.py build their corpora of valid and malformed blobs with them.
  * signals from fields: svb_signal(codes, rng) walks int16 samples whose i-th zig-zag delta needs exactly codes[i] + 1 bytes;
    exzd_signal(N, q, y0, pos, vals, rest) rebuilds the samples from the fields of an ex-zd blob, exzd_rest plans the one-byte deltas that
    carry the walk to where the next exception can happen.  A test states the bytes it wants, the signal follows, and the expectation —
    svb_blob(codes, z) or exzd_blob(N, q, z0, _gaps(pos), vals, rest) — never passes through an encoder
    (tests/test_signal_encode_craft.py).

Four-byte gaps and values of ex-zd (and four-byte svb-zd values) cannot come out of int16 samples short of a read of 2^24 samples (a gap)
or at all (a value: z <= 131070); they are left out.
"""
import struct

import numpy as np

WIDTH_LO = np.array([0, 1 << 8, 1 << 16, 1 << 24], dtype=np.uint64)      # smallest z that needs code + 1 bytes
WIDTH_END = np.array([1 << 8, 1 << 16, 1 << 24, 1 << 32], dtype=np.uint64)
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- svb-zd: blob builder and reference

def svb_blob(codes, zs, count=None, tail=b""):
    """u32 count | ceil(len/4) key bytes (2 bits per value, LSB first) | code + 1 little-endian bytes of each z.  The pairs
    (codes[i], zs[i]) are written as given: z must fit its width, a wider width than needed is allowed.  count overrides the
    count field (malformed blobs); tail is appended behind the data."""
    codes = np.asarray(codes, dtype=np.uint8)
    zs = np.asarray(zs, dtype=np.uint64)
    assert codes.shape == zs.shape and (codes <= 3).all()
    assert (zs < WIDTH_END[codes]).all()
    n = len(codes)
    padded = np.zeros(4 * ((n + 3) // 4), dtype=np.uint8)
    padded[:n] = codes
    keys = padded[0::4] | (padded[1::4] << 2) | (padded[2::4] << 4) | (padded[3::4] << 6)
    zb = zs.astype("<u4").view(np.uint8).reshape(-1, 4)
    data = zb[np.arange(4)[None, :] <= codes[:, None]]
    return struct.pack("<I", n if count is None else count) + keys.astype(np.uint8).tobytes() + data.tobytes() + bytes(tail)


def svb_ref_decode(blob):
    """int16 samples of a well-formed blob, None for a malformed one (count, keys and data bytes must add up to the length)"""
    b = np.frombuffer(bytes(blob), dtype=np.uint8)
    if len(b) < 4:
        return None
    n = int.from_bytes(bytes(b[:4]), "little")
    nk = (n + 3) // 4
    if 4 + nk > len(b):
        return None
    codes = ((b[4:4 + nk, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:n].astype(np.int64)
    end = np.cumsum(codes + 1)
    if 4 + nk + (int(end[-1]) if n else 0) != len(b):
        return None
    data = b[4 + nk:]
    start = end - (codes + 1)
    z = np.zeros(n, dtype=np.int64)
    for k in range(4):
        m = codes >= k
        z[m] |= data[start[m] + k].astype(np.int64) << (8 * k)
    d = (z >> 1) ^ -(z & 1)
    return (np.cumsum(d) & 0xFFFF).astype(np.uint16).view(np.int16)


def svb_full_width(rng, codes):
    """a z for every code that needs all of its bytes (any byte for code 0)"""
    codes = np.asarray(codes, dtype=np.int64)
    lo = WIDTH_LO[codes].astype(np.float64)
    hi = WIDTH_END[codes].astype(np.float64)
    return np.minimum(lo + np.floor(rng.random(len(codes)) * (hi - lo)), hi - 1).astype(np.uint64)


def _interleave(items, guards):
    """guard, item, guard, item, ..., guard: every item has valid neighbours on both sides"""
    out = [guards[0]]
    for it, g in zip(items, guards[1:]):
        out += [it, g]
    return out


# ---------------------------------------------------------------- ex-zd: blob builder and reference

def _min_codes(v):
    v = np.asarray(v, dtype=np.uint64)
    return ((v > 0xFF).astype(np.uint8) + (v > 0xFFFF) + (v > 0xFFFFFF)).astype(np.uint8)


def svb32(vals, codes=None):
    """ceil(len/4) key bytes (2 bits per value, LSB first) | code + 1 little-endian bytes of each value, as given: a value must
    fit its width, a wider width than needed is allowed"""
    vals = np.asarray(vals, dtype=np.uint64)
    codes = _min_codes(vals) if codes is None else np.asarray(codes, dtype=np.uint8)
    assert codes.shape == vals.shape and (codes <= 3).all()
    assert (vals < np.array(WIDTH_END, dtype=np.uint64)[codes]).all()
    n = len(vals)
    padded = np.zeros(4 * ((n + 3) // 4), dtype=np.uint8)
    padded[:n] = codes
    keys = padded[0::4] | (padded[1::4] << 2) | (padded[2::4] << 4) | (padded[3::4] << 6)
    vb = vals.astype("<u4").view(np.uint8).reshape(-1, 4)
    data = vb[np.arange(4)[None, :] <= codes[:, None]]
    return keys.astype(np.uint8).tobytes() + data.tobytes()


def exzd_blob(N, q, z0, gaps, vals, rest, gap_codes=None, val_codes=None, nex=None, slack=(b"", b""), version=0):
    """docs/codecs.md §4.4, written as given: u8 version | u64 N | u8 q | (nothing more for N == 0 without lists and rest) u16 z0 |
    u32 nex | [u32 len | svb32(gaps) + slack[0] | u32 len | svb32(vals) + slack[1]] when there are lists | rest.
    gaps = first position, then gap - 1; vals = z - 256.  nex overrides the count field; slack sits behind a section's data,
    inside its length."""
    out = struct.pack("<BQB", version, N, q)
    rest = bytes(rest)
    if N == 0 and not len(gaps) and not len(vals) and not rest and nex is None:
        return out
    out += struct.pack("<HI", z0, len(gaps) if nex is None else nex)
    if len(gaps) or len(vals):
        for lst, codes, sl in ((gaps, gap_codes, slack[0]), (vals, val_codes, slack[1])):
            sec = svb32(lst, codes) + bytes(sl)
            out += struct.pack("<I", len(sec)) + sec
    return out + rest


def _svb32_read(sec, n):
    """the n values of a section that must be consumed exactly, or None"""
    nk = (n + 3) // 4
    if nk > len(sec):
        return None
    keys = np.frombuffer(sec[:nk], dtype=np.uint8)
    codes = ((keys[:, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:n].astype(np.int64)
    end = np.cumsum(codes + 1)
    if nk + int(end[-1]) != len(sec):
        return None
    data = np.frombuffer(sec[nk:], dtype=np.uint8)
    start = end - (codes + 1)
    v = np.zeros(n, dtype=np.int64)
    for k in range(4):
        m = codes >= k
        v[m] |= data[start[m] + k].astype(np.int64) << (8 * k)
    return v


def _decode(blob):
    """(int16 samples, largest |y|) of a well-formed blob, None for a malformed one"""
    b = bytes(blob)
    L = len(b)
    if L < 10 or b[0] != 0:
        return None
    N, q = struct.unpack_from("<QB", b, 1)
    if N == 0:
        return (np.zeros(0, np.int16), 0) if L == 10 else None
    if q > 15 or L < 16 or N > 0xFFFFFFF0:
        return None
    z0, nex = struct.unpack_from("<HI", b, 10)
    if nex > N - 1:
        return None
    p = 16
    lists = []
    if nex:
        for _ in range(2):
            if p + 4 > L:
                return None
            sl = struct.unpack_from("<I", b, p)[0]
            p += 4
            if sl > L - p:
                return None
            v = _svb32_read(b[p:p + sl], nex)
            if v is None:
                return None
            lists.append(v)
            p += sl
    if L - p != N - 1 - nex:       # from here on N - 1 <= L - 16: nothing below is sized by an impossible count
        return None
    np_ = N - 1
    z = np.zeros(np_, dtype=np.int64)
    plain = np.ones(np_, dtype=bool)
    if nex:
        pos = -1
        where = []
        for g in lists[0].tolist():          # Python integers: no wrap
            pos += 1 + g
            if pos >= np_:
                return None
            where.append(pos)
        where = np.array(where, dtype=np.int64)
        plain[where] = False
        z[where] = (lists[1] + 256) & M32
    z[plain] = np.frombuffer(b[p:], dtype=np.uint8)
    d = (z >> 1) ^ -(z & 1)
    y0 = (z0 >> 1) ^ -(z0 & 1)
    y = np.concatenate([[y0], y0 + np.cumsum(d)]).astype(np.int64)
    return ((y << q) & 0xFFFF).astype(np.uint16).view(np.int16), int(np.abs(y).max())


def exzd_ref_decode(blob):
    """int16 samples of a well-formed blob, None for a malformed one: every section consumed exactly, positions summed in Python
    integers and below N - 1, z = val + 256 modulo 2^32, output (y << q) & 0xFFFF"""
    r = _decode(blob)
    return None if r is None else r[0]


def fields(x, q=None):
    """(N, q, z0, gaps, vals, rest) of a signal; q = None: the encoders' choice, the trailing zero bits common to all samples"""
    x = np.asarray(x, dtype=np.int16)
    n = len(x)
    if q is None:
        acc = int(np.bitwise_or.reduce(x.view(np.uint16))) if n else 0
        q = (acc & -acc).bit_length() - 1 if acc else 0
    if n == 0:
        return 0, q, 0, [], [], b""
    y = x.astype(np.int64) >> q
    d = np.diff(y)
    z = ((d << 1) ^ (d >> 63)) & M32
    ex = np.flatnonzero(z > 255)
    gaps = np.diff(np.concatenate([[-1], ex])) - 1
    z0 = int((y[0] << 1) ^ (y[0] >> 63)) & 0xFFFF
    return n, q, z0, gaps, z[ex] - 256, z[z <= 255].astype(np.uint8).tobytes()


def _gaps(pos):
    pos = np.asarray(pos, dtype=np.int64)
    return np.diff(np.concatenate([[-1], pos])) - 1


def _balance(vals, run=0):
    """set the low bit of every val (the sign of its delta: val and z = val + 256 have the same parity) against the running sum
    of the exceptions' deltas, so that |y| stays far below 2^31 (the oracle accumulates in int32); run: where the sum starts"""
    out = []
    for v in np.asarray(vals, dtype=np.uint64).tolist():
        v = (v & ~1) | (1 if run > 0 else 0)
        z = (v + 256) & M32
        run += (z >> 1) ^ -(z & 1)
        out.append(v)
    return np.array(out, dtype=np.uint64)


# ---------------------------------------------------------------- signals from fields

def zigzag(d):
    d = np.asarray(d, dtype=np.int64)
    return ((d << 1) ^ (d >> 63)) & M32


def unzigzag(z):
    z = np.asarray(z, dtype=np.int64)
    return (z >> 1) ^ -(z & 1)


def svb_fields(x):
    """(codes, z) of int16 samples: z = zig-zag of x[i] - x[i-1] with x[-1] = 0, at its minimal width"""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    z = zigzag(np.diff(np.concatenate([[0], x]))).astype(np.uint64)
    return _min_codes(z), z


def svb_signal(codes, rng, lo=-32768, hi=32767, z_at=None):
    """(x int16, z): a walk from x[-1] = 0 inside [lo, hi] whose i-th zig-zag delta needs exactly codes[i] + 1 bytes (codes 0, 1, 2).
    Code 2 means |delta| >= 32768: the walk must stand on the far side of zero, so it never rests on 0 in front of a code-2 value, and the
    first value of a read cannot be code 2.  z_at: {i: z} values given exactly (each must fit its code and the walk)."""
    codes = np.asarray(codes, dtype=np.int64)
    n = len(codes)
    z_at = z_at or {}
    u = rng.random(n)
    side = rng.random(n) < 0.5
    x = np.zeros(n, dtype=np.int64)
    prev = 0
    cl = codes.tolist()
    for i, c in enumerate(cl):
        nxt2 = i + 1 < n and cl[i + 1] == 2
        if i in z_at:
            v = prev + int(unzigzag(z_at[i]))
            assert lo <= v <= hi and not (nxt2 and v == 0), (i, prev, v)
        else:
            if c == 0:
                ranges = [(max(lo, prev - 128), min(hi, prev + 127))]
            elif c == 1:
                ranges = [(max(lo, prev - 32768), min(hi, prev - 129)), (max(lo, prev + 128), min(hi, prev + 32767))]
            else:
                assert c == 2 and prev != 0, (i, c, prev)
                ranges = [(max(lo, prev - 65535), min(hi, prev - 32769)), (max(lo, prev + 32768), min(hi, prev + 65535))]
            ranges = [r for r in ranges if r[0] <= r[1] and not (nxt2 and r == (0, 0))]
            assert ranges, (i, c, prev)
            a, b = ranges[1 if len(ranges) > 1 and side[i] else 0]
            v = a + int(u[i] * (b - a + 1))
            if nxt2 and v == 0:
                v = a if a != 0 else b
        x[i] = prev = v
    xs = x.astype(np.int16)
    got_codes, z = svb_fields(xs)
    assert np.array_equal(got_codes, codes), "the walk does not give the codes asked for"
    for i, v in z_at.items():
        assert int(z[i]) == v
    return xs, z


def exzd_signal(N, q, y0, pos, vals, rest):
    """x int16 of the fields: z = val + 256 on the positions pos (position p is the step from sample p to sample p + 1), the bytes of rest
    on all others, y rebuilt from y0 by the zig-zag deltas, x = y << q.  Asserts that x stays in int16 and that q is the canonical choice:
    some sample has bit q set and none a lower one (q = 0 for an all-zero read)."""
    if N == 0:
        assert not len(pos) and not len(vals) and not len(rest) and q == 0
        return np.zeros(0, dtype=np.int16)
    pos = np.asarray(pos, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.int64)
    assert len(pos) == len(vals) and len(rest) == N - 1 - len(pos) and (np.diff(pos) > 0).all()
    assert not len(pos) or (pos[0] >= 0 and pos[-1] < N - 1)
    z = np.zeros(N - 1, dtype=np.int64)
    plain = np.ones(N - 1, dtype=bool)
    plain[pos] = False
    z[pos] = vals + 256
    z[plain] = np.frombuffer(bytes(rest), dtype=np.uint8)
    y = np.concatenate([[y0], y0 + np.cumsum(unzigzag(z))]).astype(np.int64)
    x = y << q
    assert x.min() >= -32768 and x.max() <= 32767, (int(x.min()), int(x.max()))
    acc = int(np.bitwise_or.reduce(x & 0xFFFF))
    assert (q == 0 and acc == 0) or (acc & -acc) == 1 << q, (q, acc)
    return x.astype(np.int16)


def exzd_z0(y0):
    return int(zigzag(y0)) & 0xFFFF


def exzd_rest(N, q, y0, pos, vals, rng, wander=24, force=None):
    """the one-byte z of every position that is no exception, planned so that the walk y stays inside what q leaves of int16 and stands,
    in front of every exception, where that exception's delta can be added: between two exceptions y moves along a straight line to the
    nearest such place (at most 72 per step) with a little noise on top (at most `wander` either way, none on the last step).
    force: {position: z <= 255} bytes of rest given exactly; the walk is led to them in the same way."""
    lo, hi = -(32768 >> q), 32767 >> q
    pos = np.asarray(pos, dtype=np.int64)
    dex = unzigzag(np.asarray(vals, dtype=np.int64) + 256)
    events = [(p, D, True) for p, D in zip(pos.tolist(), dex.tolist())]
    events += [(p, int(unzigzag(z)), False) for p, z in (force or {}).items()]
    assert len({p for p, _, _ in events}) == len(events) and all(z <= 255 for z in (force or {}).values())
    out = []
    y, at = int(y0), 0                       # the walk's value at sample `at`
    assert lo <= y <= hi
    for p, D, is_ex in sorted(events) + [(N - 1, 0, True)]:
        m = p - at                           # free steps in front of this one
        wlo, whi = max(lo, lo - D), min(hi, hi - D)
        assert wlo <= whi, (p, D)
        b = min(max(y, wlo), whi)
        assert abs(b - y) <= 72 * m, ("the walk cannot reach the step at", p, y, b, m)
        if m:
            i = np.arange(1, m + 1, dtype=np.int64)
            w = rng.integers(-wander, wander + 1, m)
            w[-1] = 0
            path = np.clip(y + (b - y) * i // m + w, lo, hi)
            d = np.diff(np.concatenate([[y], path]))
            assert d.min() >= -128 and d.max() <= 127
            out.append(zigzag(d).astype(np.uint8))
        if not is_ex:
            out.append(zigzag([D]).astype(np.uint8))
        y = b + D
        at = p + 1
    return np.concatenate(out).tobytes() if out else b""
