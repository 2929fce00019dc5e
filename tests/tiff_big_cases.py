"""Segments of the size a scene has, for the TIFF reader's decoders: one case table that tests/test_tiff_host_big.py runs through
the host build of csrc/tiff.inc and tests/test_gpu_tiff_big.py on the device.  No fixtures: everything is generated from
seeds.  The expected bytes of a row are the plain reference -- the input that was compressed, or, for the streams assembled
by hand here, the bytes the Deflater kept while it wrote them -- and zlib is the independent judge of every Deflate stream,
hand-made ones included, before a row leaves this module.  TEST INFRASTRUCTURE.

    rows()           [(name, codec, stream, expected bytes)]: sound streams; status 0 and exactly these bytes
    damage_rows()    [(name, codec, damaged stream, want, sound stream, expected bytes)]: segments longer than the history
                     ring, damaged; want: the status it must end in, None for any non-zero one
    ADLER_DATA()     non-zero data longer than 65521 and than 2 x 65521 bytes, for the Adler-32 alone

What the rows are for (csrc/tiff.inc): Deflate's history is a ring of 32768 bytes that 64 lanes read and write in the same
step, so matches at distances within 258 of the ring's size, matches that cross a multiple of 32768, matches into stored
blocks (which fill the ring for their last 32768 bytes only), codes longer than the fast tables' 10 / 9 bits, a stop at the
expected size beyond the first trip round the ring, and Adler weights that wrap at 65521 on non-zero data; LZW's table
through many lifetimes, strings of hundreds of bytes and a table that fills and is never cleared; PackBits runs of every
length."""
import functools
import zlib

import numpy as np

import tiff_reference as R

RING = 32768
CAP_DEFLATE, CAP_LZW = 768 << 10, 384 << 10      # lbdrn_tiff_segment_cap(8) and (5): the tests assert that they are


def base_raster_like(C, H, W, seed):
    """tests/test_tiff_host.py's base_raster at another size: a random walk along each row, a row of noise, two constant rows"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.integers(-60, 61, (C, H, W)), axis=2) + rng.integers(0, 65536, (C, H, 1))
    a[:, 3, :] = rng.integers(0, 65536, (C, W))
    a[:, 7:9, :] = 513
    return (a % 65536).astype(np.uint16)


def periodic_noise(period, n, seed):
    return (np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8).tobytes() * (n // period + 1))[:n]


# ---------------------------------------------------------------- Deflate blocks by hand

_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in (0, 1))
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_FIXED_LIT = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8


def canonical(lens):
    """{symbol: (the code's bits in stream order, its length)} of RFC 1951's canonical code for these lengths"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (int(format(nxt[n], f"0{n}b")[::-1], 2), n)
            nxt[n] += 1
    return out


class Deflater:
    """A zlib stream block by block: stored, fixed and dynamic blocks with the code lengths the caller gives, literals and
    matches as told.  `data` is what the stream decodes to; `longest` holds the longest literal/length and distance codes
    that were written into the data (not merely declared)."""

    def __init__(self):
        self.w = R._LsbWriter()
        self.data = bytearray()
        self.lit = self.dist = None
        self.longest = [0, 0]

    def stored(self, payload, last=False, claim=None):
        """claim: the LEN the header states, where it is not the payload's"""
        w = self.w
        w.bits(1 if last else 0, 1)
        w.bits(0, 2)
        if w.nbits:
            w.bits(0, 8 - w.nbits)
        n = len(payload) if claim is None else claim
        w.bits(n, 16)
        w.bits(n ^ 0xFFFF, 16)
        w.out += payload
        self.data += payload

    def block(self, last=False, lit_lens=None, dist_lens=None):
        """open a fixed block, or a dynamic one whose header states these lengths (each in four bits: a code length code of
        sixteen 4-bit codes for the lengths 0 .. 15, no repeat codes)"""
        w = self.w
        w.bits(1 if last else 0, 1)
        if lit_lens is None:
            w.bits(1, 2)
            lit_lens, dist_lens = _FIXED_LIT, (5,) * 30
        else:
            w.bits(2, 2)
            assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30 and lit_lens[256]
            w.bits(len(lit_lens) - 257, 5)
            w.bits(len(dist_lens) - 1, 5)
            w.bits(19 - 4, 4)
            cl = [4] * 16 + [0] * 3
            for s in _CL_ORDER:
                w.bits(cl[s], 3)
            codes = canonical(cl)
            for n in tuple(lit_lens) + tuple(dist_lens):
                w.bits(*codes[n])
        self.lit, self.dist = canonical(lit_lens), canonical(dist_lens)

    def literals(self, data):
        w, lit = self.w, self.lit
        for b in data:
            w.bits(*lit[b])
            self.longest[0] = max(self.longest[0], lit[b][1])
        self.data += data

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= min(RING, len(self.data)), (length, dist, len(self.data))
        w = self.w
        li = max(i for i, b in enumerate(_LEN_BASE) if b <= length)
        w.bits(*self.lit[257 + li])
        w.bits(length - _LEN_BASE[li], _LEN_EXTRA[li])
        di = max(i for i, b in enumerate(_DIST_BASE) if b <= dist)
        w.bits(*self.dist[di])
        w.bits(dist - _DIST_BASE[di], _DIST_EXTRA[di])
        self.longest = [max(self.longest[0], self.lit[257 + li][1]), max(self.longest[1], self.dist[di][1])]
        at = len(self.data) - dist
        for i in range(length):
            self.data.append(self.data[at + i])

    def end(self):
        self.w.bits(*self.lit[256])
        self.longest[0] = max(self.longest[0], self.lit[256][1])

    def pad_to(self, target, rng):
        """matches of length 258 at far distances, then literals, until the output is `target` bytes long"""
        while len(self.data) + 258 <= target:
            self.match(258, RING - int(rng.integers(0, 600)))
        self.literals(rng.integers(0, 256, target - len(self.data), dtype=np.uint8).tobytes())

    def finish(self):
        return b"\x78\x9c" + self.w.finish() + zlib.adler32(bytes(self.data)).to_bytes(4, "big")


def dynamic_code_lengths(stream):
    """(literal/length lengths, distance lengths) that the header of a zlib stream's first block states; None where that block
    is not a dynamic one.  Shows which code lengths a stream zlib made asks of a decoder."""
    bits = int.from_bytes(stream[2:2 + 400], "little")
    at = 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v
    take(1)
    if take(2) != 2:
        return None
    nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for s in _CL_ORDER[:ncode]:
        cl[s] = take(3)
    by_code = {v: s for s, v in canonical(cl).items()}
    lens = []
    while len(lens) < nlen + ndist:
        code, n = 0, 0
        while (code, n) not in by_code:
            code |= take(1) << n
            n += 1
            assert n <= 7
        s = by_code[(code, n)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * (3 + take(3) if s == 17 else 11 + take(7))
    return lens[:nlen], lens[nlen:nlen + ndist]


def _judged(d, expect=None):
    """(stream, expected bytes) of a finished Deflater, after zlib has decoded the stream to the bytes the Deflater kept"""
    stream, data = d.finish(), bytes(d.data)
    z = zlib.decompressobj()
    assert z.decompress(stream) == data and z.eof and not z.unused_data, "zlib reads a hand-made stream otherwise"
    return stream, data if expect is None else data[:expect]


def _hand_fixed_far():
    """fixed code: 32768 + 300 literals, then matches of length 258, 3 and 65 at distances 32768, 32767, 32768 - 63, - 64, - 257
    and - 258; a far match inside which the output crosses 2 x 32768; overlapping matches (distance 1, 2, 63, 64, 65, length
    258) that straddle the next five multiples of 32768"""
    rng = np.random.default_rng(21)
    d = Deflater()
    d.block(last=True)
    d.literals(rng.integers(0, 256, RING + 300, dtype=np.uint8).tobytes())
    for length in (258, 3, 65):
        for dist in (RING, RING - 1, RING - 63, RING - 64, RING - 257, RING - 258):
            d.match(length, dist)
    d.pad_to(2 * RING - 100, rng)
    d.match(258, RING - 31)
    assert len(d.data) == 2 * RING + 158
    for k, dist in enumerate((1, 2, 63, 64, 65)):
        d.pad_to((3 + k) * RING - 129, rng)
        d.match(258, dist)
        assert len(d.data) == (3 + k) * RING + 129
    d.literals(b"end")
    d.end()
    return _judged(d)


def _hand_stored_then_match():
    """two stored blocks of 65535 bytes, then a fixed block whose first match begins at the oldest byte the ring may hold
    (distance 32768), then 32767, then 1: all three read stored bytes"""
    rng = np.random.default_rng(22)
    d = Deflater()
    for _ in range(2):
        d.stored(rng.integers(0, 256, 65535, dtype=np.uint8).tobytes())
    d.block(last=True)
    d.match(258, RING)
    d.match(258, RING - 1)
    d.match(258, 1)
    d.match(3, RING)
    d.literals(b"tail")
    d.end()
    return _judged(d)


def _hand_stored_inside_ring():
    """40000 literals, a stored block of 20000 bytes, then matches into both: the ring holds the stored block and the last
    12768 literals in front of it"""
    rng = np.random.default_rng(23)
    d = Deflater()
    d.block()
    d.literals(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())
    d.end()
    d.stored(rng.integers(0, 256, 20000, dtype=np.uint8).tobytes())
    d.block(last=True)
    for dist in (RING, 20001, 20000, 19999, RING - 63, 1, 25000):
        d.match(258, dist)
        d.match(3, dist)
    d.end()
    return _judged(d)


_LONG = tuple(range(1, 15)) + (15, 15)      # a complete code: 2^-1 + ... + 2^-14 + 2 x 2^-15 = 1


def _hand_long_literal_codes():
    """two dynamic blocks whose literal/length code has the lengths 1, 2, ..., 14, 15, 15: fourteen literals with 1 to 14 bits,
    the end-of-block code and the length-3 code with 15"""
    rng = np.random.default_rng(24)
    values = [int(v) for v in rng.permutation(256)[:14]]
    lit = [0] * 258
    for v, n in zip(values, _LONG):
        lit[v] = n
    lit[256] = lit[257] = 15
    d = Deflater()
    for last in (False, True):
        d.block(last=last, lit_lens=lit, dist_lens=(1, 1))
        for k in range(3000):
            d.literals(bytes(values[int(i)] for i in rng.integers(0, 14, 7)))
            d.literals(bytes(values[10:]))      # the 11- to 14-bit codes, every time
            if k % 3 == 0:
                d.match(3, 1 + k % 2)
        d.end()
    assert d.longest[0] == 15 > 10
    return _judged(d)


def _hand_long_distance_codes():
    """a dynamic block whose distance code has the lengths 1, 2, ..., 14, 15, 15 over sixteen distance symbols, near and far;
    every one of them is used, the 10- to 15-bit ones by matches of length 3 and 258"""
    rng = np.random.default_rng(25)
    symbols = (29, 0, 28, 1, 27, 2, 3, 26, 4, 25, 10, 20, 15, 5, 24, 12)
    dist = [0] * 30
    for s, n in zip(symbols, _LONG):
        dist[s] = n
    lit = [9] * 256 + [2, 3] + [0] * 27 + [3]      # 256 x 2^-9 + 2^-2 + 2 x 2^-3 = 1
    d = Deflater()
    d.block(last=True, lit_lens=lit, dist_lens=dist)
    d.literals(rng.integers(0, 256, RING + 500, dtype=np.uint8).tobytes())
    for rnd in range(6):
        for s in symbols:
            d.match((3, 258)[rnd % 2], _DIST_BASE[s] + int(rng.integers(0, 1 << _DIST_EXTRA[s])))
        d.literals(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
    d.end()
    assert d.longest[1] == 15 > 9
    return _judged(d)


def _hand_stop_early():
    """streams that hold more than the segment; the segment ends beyond the first trip round the ring, in a literal run, inside a
    match and inside a stored block"""
    rng = np.random.default_rng(26)
    out = []
    d = Deflater()
    d.block(last=True)
    d.literals(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())
    d.end()
    out.append(("stop-in-literals", _judged(d, 39000)))
    d = Deflater()
    d.block(last=True)
    d.literals(rng.integers(0, 256, 33000, dtype=np.uint8).tobytes())
    d.match(258, RING)
    d.match(258, 7)
    d.end()
    out.append(("stop-in-match", _judged(d, 33100)))
    d = Deflater()
    d.stored(rng.integers(0, 256, 50000, dtype=np.uint8).tobytes())
    d.stored(rng.integers(0, 256, 50000, dtype=np.uint8).tobytes(), last=True)
    out.append(("stop-in-stored", _judged(d, 90000)))
    return out


def skewed_source(n=200000, seed=27):
    """forty symbols, each 0.8 times as frequent as the one before it: zlib gives the rare ones codes of more than ten bits"""
    rng = np.random.default_rng(seed)
    p = 0.8 ** np.arange(40)
    return rng.choice(np.arange(40, dtype=np.uint8) * 5 + 3, n, p=p / p.sum()).tobytes()


def _zlib(data, level):
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED) if level == "fixed" else zlib.compressobj(level)
    return c.compress(data) + c.flush()


def ADLER_DATA():
    rng = np.random.default_rng(28)
    return (b"\xff" * 65522, b"\xff" * (2 * 65521 + 1), rng.integers(1, 256, 140001, dtype=np.uint8).tobytes())


# ---------------------------------------------------------------- PackBits by hand

def _packbits_every_run(n=1 << 20, seed=29):
    """literal runs of 1 .. 128 bytes and replicate runs of 2 .. 128 (the format has no shorter one), in a seeded order, with a
    no-op byte in front of every seventh run"""
    rng = np.random.default_rng(seed)
    stream, data = bytearray(), bytearray()
    runs = [(kind, k) for k in range(1, 129) for kind in (0, 1) if kind == 0 or k > 1]
    i = 0
    while len(data) < n:
        if i % len(runs) == 0:
            order = rng.permutation(len(runs))
        kind, k = runs[int(order[i % len(runs)])]
        k = min(k, n - len(data))
        if kind and k < 2:
            kind = 0
        if i % 7 == 0:
            stream.append(0x80)
        if kind:
            v = int(rng.integers(0, 256))
            stream += bytes([257 - k, v])
            data += bytes([v]) * k
        else:
            part = rng.integers(0, 256, k, dtype=np.uint8).tobytes()
            stream.append(k - 1)
            stream += part
            data += part
        i += 1
    stream.append(0x80)
    assert i > 2 * len(runs) and R.packbits_decode(bytes(stream), n) == bytes(data)
    return bytes(stream), bytes(data)


# ---------------------------------------------------------------- the table

def _smooth16(nbytes, seed, byteorder="<"):
    """a 256-sample-wide raster of smooth 16-bit data as one segment of nbytes, after the horizontal predictor"""
    a = base_raster_like(1, nbytes // 512, 256, seed)
    (seg,) = R.raw_segments(a, rows_per_strip=a.shape[1], predictor=2, byteorder=byteorder)
    assert len(seg) == nbytes
    return seg


@functools.lru_cache(maxsize=None)
def rows():
    out = []
    D, L, P = R.COMP_DEFLATE, R.COMP_LZW, R.COMP_PACKBITS
    # 1. what zlib writes for segments of a scene's size: hash chains, lazy matches, distances up to 32506, dynamic codes
    tile = R.raw_segments(base_raster_like(1, 256, 256, 31), tile=(256, 256), predictor=2)[0]
    chunky = R.raw_segments(base_raster_like(8, 128, 128, 32), tile=(128, 128), planar=1, predictor=2)[0]
    assert len(tile) == 128 << 10 and len(chunky) == 256 << 10
    far = {}
    for name, data in (("period32506", periodic_noise(32506, 128 << 10, 33)), ("period20000-cap", periodic_noise(20000, CAP_DEFLATE, 34)),
                       ("tile256", tile), ("chunky8x128", chunky)):
        for level in (1, 6, 9, "fixed"):
            far[name, level] = _zlib(data, level)
            out.append((f"zlib-{name}-{level}", D, far[name, level], data))
    assert len(far["period32506", 9]) < 40000 and len(far["period20000-cap", 6]) < 40000      # (the far matches are found)
    # 2. - 5. hand-made streams
    out.append(("hand-fixed-far-matches", D) + _hand_fixed_far())
    out.append(("hand-stored-then-match", D) + _hand_stored_then_match())
    out.append(("hand-stored-inside-ring", D) + _hand_stored_inside_ring())
    out.append(("hand-long-literal-codes", D) + _hand_long_literal_codes())
    out.append(("hand-long-distance-codes", D) + _hand_long_distance_codes())
    skew = skewed_source()
    out.append(("zlib-skewed-9", D, _zlib(skew, 9), skew))
    assert max(dynamic_code_lengths(out[-1][2])[0]) > 10      # the natural companion: zlib's own code is longer than the fast table
    out += [(name, D) + pair for name, pair in _hand_stop_early()]
    # 6. Adler-32 on non-zero data whose weights wrap once and twice
    for k, data in enumerate(ADLER_DATA()):
        out.append((f"adler-{len(data)}", D, _zlib(data, 6), data))
    for name, codec, stream, expected in out:      # zlib judges every Deflate row
        z = zlib.decompressobj()
        got = z.decompress(stream)
        assert z.eof and not z.unused_data and got[:len(expected)] == expected and (len(got) == len(expected)) == (not name.startswith("stop-")), name
    # LZW
    rng = np.random.default_rng(35)
    noise = rng.integers(0, 256, CAP_LZW, dtype=np.uint8).tobytes()
    out.append(("lzw-noise-cap", L, R.lzw_encode(noise), noise))
    const = b"\x21" * CAP_LZW      # strings of 1, 2, 3, ... bytes: the 886th reaches the cap, and the table never fills
    codes = R.lzw_code_list(const)
    assert len(codes) < 900 and [c for c, _ in codes[2:-2]] == list(range(258, 258 + len(codes) - 4))
    out.append(("lzw-constant-cap", L, R.lzw_pack(codes), const))
    four = rng.integers(0, 4, 60000, dtype=np.uint8).tobytes()      # four symbols: the table is full after a third of it
    codes = R.lzw_code_list(four, clear=False)
    assert [c for c, _ in codes].count(R.CLEAR) == 1 and len(codes) > 2 * (4096 - 258) and codes[-2][1] == 12
    out.append(("lzw-full-table-no-clear", L, R.lzw_pack(codes), four))
    smooth = _smooth16(CAP_LZW, 36, ">")
    out.append(("lzw-smooth16-cap", L, R.lzw_encode(smooth), smooth))
    for name, codec, stream, expected in out[-4:]:
        assert R.lzw_decode(stream, len(expected)) == expected, name
    # PackBits
    out.append(("packbits-every-run", P) + _packbits_every_run())
    assert len({r[0] for r in out}) == len(out)
    return tuple(out)


# ---------------------------------------------------------------- damage at size

def _cut_after(stream, nbytes):
    """the shortest prefix of a zlib stream that still yields nbytes of output"""
    lo, hi = 0, len(stream)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(zlib.decompressobj().decompress(stream[:mid])) >= nbytes:
            hi = mid
        else:
            lo = mid + 1
    return stream[:lo]


@functools.lru_cache(maxsize=None)
def damage_rows():
    """Damaged segments longer than the ring.  Each must end in a status and never in the expected bytes; `want` names the
    status where the stream stays well-formed and only its check can tell."""
    D, L = R.COMP_DEFLATE, R.COMP_LZW
    table = {r[0]: r for r in rows()}
    out = []
    _, _, sound, data = table["zlib-tile256-6"]
    for n in (40000, 100000):
        out.append((f"deflate-cut-after-{n}", D, _cut_after(sound, n), None, sound, data))
    at = 8 * (len(sound) * 3 // 4) + 3
    flipped = bytearray(sound)
    flipped[at >> 3] ^= 1 << (at & 7)
    out.append(("deflate-bit-flip-late", D, bytes(flipped), None, sound, data))
    # the same match at another distance, under the first stream's check: both distances are symbol 29 with 13 more bits
    rng = np.random.default_rng(41)
    head = rng.integers(0, 256, 33000, dtype=np.uint8).tobytes()
    pair = []
    for dist in (RING, RING - 1):
        d = Deflater()
        d.block(last=True)
        d.literals(head)
        d.match(258, dist)
        d.literals(b"after")
        d.end()
        pair.append(_judged(d))
    (good, good_data), (other, other_data) = pair
    assert len(good) == len(other) and good_data != other_data
    out.append(("deflate-other-distance", D, other[:-4] + good[-4:], 5, good, good_data))
    d = Deflater()      # a stored block that states 65535 bytes and has 50000, behind 40000 literals
    d.block()
    d.literals(head + head[:7000])
    d.end()
    d.stored(head + head[:17000], last=True, claim=65535)
    sound_d = Deflater()
    sound_d.block(last=True)
    sound_d.literals((head * 4)[:40000 + 65536])
    sound_d.end()
    out.append(("deflate-stored-len-past-stream", D, d.finish()[:-4], 1) + _judged(sound_d))
    # LZW: late in a segment of many table lifetimes
    _, _, sound, data = table["lzw-smooth16-cap"]
    codes = R.lzw_code_list(data)
    clears = [i for i, (c, _) in enumerate(codes) if c == R.CLEAR]
    assert len(clears) > 20
    late = clears[len(clears) * 3 // 4]
    bad = list(codes)
    assert bad[late + 10][1] == 9
    bad[late + 10] = (400, 9)      # ten codes after a Clear the table ends at 266
    out.append(("lzw-code-above-next-late", L, R.lzw_pack(bad), 2, sound, data))
    bad = list(codes)
    bad[late + 300] = (R.EOI, bad[late + 300][1])
    out.append(("lzw-eoi-late", L, R.lzw_pack(bad), 1, sound, data))
    for name, codec, bad, want, sound, data in out:      # the reference refuses every one of them
        try:
            got = R.decompress(bad, codec, len(data))
        except (ValueError, zlib.error):
            continue
        raise AssertionError(f"{name}: the reference reads it: {got == data}")
    return tuple(out)
