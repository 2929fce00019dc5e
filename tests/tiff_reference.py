"""TIFF restated from its specification for the tests of the GPU reader: a writer for every layout the reader takes, a
textbook TIFF-LZW encoder and decoder, PackBits both ways, Deflate through zlib, and the placement of decoded segments in
numpy.  Plain Python; nothing is imported from the product.  TEST INFRASTRUCTURE.

The LZW encoder follows TIFF 6.0 section 13 with libtiff's "early change": a Clear first, codes MSB-first, the width grows
when the next free code reaches 512 / 1024 / 2048, a Clear when it reaches 4094, EOI last.  libtiff 4.7.1 reads what it
writes (tests/golden/make_golden_tiff.py records that check)."""
import struct
import zlib

import numpy as np

COMP_NONE, COMP_LZW, COMP_DEFLATE, COMP_DEFLATE_OLD, COMP_PACKBITS = 1, 5, 8, 32946, 32773
CLEAR, EOI = 256, 257


# ---------------------------------------------------------------- LZW

class _MsbWriter:
    def __init__(self):
        self.acc, self.nbits, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.nbits += width
        while self.nbits >= 8:
            self.nbits -= 8
            self.out.append((self.acc >> self.nbits) & 0xFF)
        self.acc &= (1 << self.nbits) - 1

    def finish(self):
        if self.nbits:
            self.out.append((self.acc << (8 - self.nbits)) & 0xFF)
        return bytes(self.out)


def lzw_code_list(data, clear=True):
    """[(code, width)] of the stream lzw_encode writes, the leading Clear and the EOI included.  clear=False: the coder never
    sends a second Clear; once the table holds its 4096 codes it adds no entry and goes on with 12-bit codes (TIFF 6.0 lets
    a writer do that; a reader's table then stays as it is)."""
    data = bytes(data)
    out = []
    table, nxt, width = {}, 258, 9
    out.append((CLEAR, width))
    cur = None      # code of the string matched so far
    for c in data:
        if cur is None:
            cur = c
            continue
        key = (cur, c)
        if key in table:
            cur = table[key]
            continue
        out.append((cur, width))
        if nxt < 4096:
            table[key] = nxt
            nxt += 1
            if nxt == 4094 and clear:
                out.append((CLEAR, width))
                table, nxt, width = {}, 258, 9
            elif nxt in (512, 1024, 2048):
                width += 1
        cur = c
    if cur is not None:
        out.append((cur, width))
        if nxt < 4096:
            nxt += 1
            if nxt == 4094 and clear:
                out.append((CLEAR, width))
                width = 9
            elif nxt in (512, 1024, 2048):
                width += 1
    out.append((EOI, width))
    return out


def lzw_pack(codes):
    """[(code, width)] -> the stream's bytes, MSB first"""
    w = _MsbWriter()
    for code, width in codes:
        w.put(code, width)
    return w.finish()


def lzw_encode(data, clear=True):
    return lzw_pack(lzw_code_list(data, clear))


def lzw_decode(data, expect):
    """the first `expect` bytes of the stream; ValueError where it is damaged or ends early"""
    data = bytes(data)
    out = bytearray()
    bit, width, table, prev = 0, 9, [], None      # table[i]: string of code 258 + i
    while len(out) < expect:
        if bit + width > 8 * len(data):
            raise ValueError("LZW stream ends early")
        code = (int.from_bytes(data[bit >> 3:(bit >> 3) + 3].ljust(3, b"\0"), "big") >> (24 - (bit & 7) - width)) & ((1 << width) - 1)
        bit += width
        if code == EOI:
            raise ValueError("EOI before the expected size")
        if code == CLEAR:
            width, table, prev = 9, [], None
            continue
        if prev is None:
            if code > 255:
                raise ValueError("bad code after Clear")
            s = bytes([code])
        else:
            if code < 256:
                s = bytes([code])
            elif code - 258 < len(table):
                s = table[code - 258]
            elif code - 258 == len(table) and len(table) < 4096 - 258:
                s = prev + prev[:1]
            else:
                raise ValueError("LZW code beyond the table")
            if len(table) < 4096 - 258:
                table.append(prev + s[:1])
                if 258 + len(table) == (1 << width) - 1 and width < 12:
                    width += 1
        out += s
        prev = s
    return bytes(out[:expect])


# ---------------------------------------------------------------- PackBits

def packbits_encode(data, row_bytes=None):
    """rows are packed separately (TIFF 6.0 section 9); replicate runs of 3 or more, up to 128; literals up to 128"""
    data = bytes(data)
    row_bytes = row_bytes or len(data) or 1
    out = bytearray()
    for r0 in range(0, len(data), row_bytes):
        row = data[r0:r0 + row_bytes]
        i, lit = 0, bytearray()

        def flush():
            for k in range(0, len(lit), 128):
                part = lit[k:k + 128]
                out.append(len(part) - 1)
                out.extend(part)
            lit.clear()
        while i < len(row):
            j = i
            while j < len(row) and row[j] == row[i] and j - i < 128:
                j += 1
            if j - i >= 3:
                flush()
                out.append(257 - (j - i))
                out.append(row[i])
                i = j
            else:
                lit.append(row[i])
                i += 1
        flush()
    return bytes(out)


def packbits_decode(data, expect):
    data = bytes(data)
    out, i = bytearray(), 0
    while len(out) < expect:
        if i >= len(data):
            raise ValueError("PackBits stream ends early")
        c = data[i]
        i += 1
        if c == 128:
            continue
        if c < 128:
            if i + c + 1 > len(data):
                raise ValueError("PackBits literal run past the stream")
            out += data[i:i + c + 1]
            i += c + 1
        else:
            if i >= len(data):
                raise ValueError("PackBits stream ends early")
            out += data[i:i + 1] * (257 - c)
            i += 1
        if len(out) > expect:
            raise ValueError("PackBits run past the segment")
    return bytes(out)


# ---------------------------------------------------------------- Deflate

DEFLATE_MODES = ("stored", "fixed", "dynamic", "multi")


def deflate(data, mode="dynamic"):
    data = bytes(data)
    if mode == "stored":
        c = zlib.compressobj(0)
    elif mode == "fixed":
        c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    else:
        c = zlib.compressobj(9)
    if mode == "multi":
        half = len(data) // 2
        return c.compress(data[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[half:]) + c.flush()
    return c.compress(data) + c.flush()


def compress(data, compression, deflate_mode="dynamic", row_bytes=None):
    if compression == COMP_NONE:
        return bytes(data)
    if compression == COMP_LZW:
        return lzw_encode(data)
    if compression in (COMP_DEFLATE, COMP_DEFLATE_OLD):
        return deflate(data, deflate_mode)
    if compression == COMP_PACKBITS:
        return packbits_encode(data, row_bytes)
    raise ValueError(compression)


def decompress(data, compression, expect):
    if compression == COMP_NONE:
        if len(data) < expect:
            raise ValueError("short segment")
        return bytes(data[:expect])
    if compression == COMP_LZW:
        return lzw_decode(data, expect)
    if compression in (COMP_DEFLATE, COMP_DEFLATE_OLD):
        out = zlib.decompress(bytes(data))
        if len(out) < expect:
            raise ValueError("short segment")
        return out[:expect]
    if compression == COMP_PACKBITS:
        return packbits_decode(data, expect)
    raise ValueError(compression)


# ---------------------------------------------------------------- segments of a raster

def segment_grid(C, H, W, tile, rows_per_strip, planar):
    """[(band or None, y0, x0, seg_h, seg_w, rows inside the image)] in TIFF order"""
    if tile:
        sw, sh = tile
    else:
        sw, sh = W, min(rows_per_strip or H, H)
    one = [(y0, x0) for y0 in range(0, H, sh) for x0 in range(0, W, sw)]
    bands = range(C) if planar == 2 else [None]
    return [(b, y0, x0, sh, sw, min(sh, H - y0)) for b in bands for y0, x0 in one]


def raw_segments(a, tile=None, rows_per_strip=None, planar=2, predictor=1, byteorder="<"):
    """the uncompressed bytes of every segment of a [C,H,W] uint8 / uint16 array: tiles padded with zeros to full size, the
    last strip short, predictor 2 applied along each segment row per sample channel on native values, then the byte order"""
    C, H, W = a.shape
    out = []
    for b, y0, x0, sh, sw, rows in segment_grid(C, H, W, tile, rows_per_strip, planar):
        hh = sh if tile else rows
        src = a[b:b + 1] if b is not None else a
        seg = np.zeros((hh, sw, src.shape[0]), a.dtype)
        part = src[:, y0:y0 + hh, x0:x0 + sw]
        seg[:part.shape[1], :part.shape[2], :] = part.transpose(1, 2, 0)
        if predictor == 2:
            seg[:, 1:, :] = seg[:, 1:, :] - seg[:, :-1, :]      # modulo 2^bits: unsigned wrap
        out.append(seg.astype(seg.dtype.newbyteorder(byteorder)).tobytes())
    return out


def place_segments(segs, C, H, W, dtype, tile=None, rows_per_strip=None, planar=2, predictor=1, byteorder="<"):
    """the inverse of raw_segments: decoded segment bytes -> [C,H,W]"""
    dtype = np.dtype(dtype)
    out = np.zeros((C, H, W), dtype)
    for raw, (b, y0, x0, sh, sw, rows) in zip(segs, segment_grid(C, H, W, tile, rows_per_strip, planar)):
        hh = sh if tile else rows
        spp = 1 if b is not None else C
        seg = np.frombuffer(raw, dtype.newbyteorder(byteorder), hh * sw * spp).astype(dtype).reshape(hh, sw, spp)
        if predictor == 2:
            seg = np.cumsum(seg, axis=1, dtype=dtype)
        cols = min(sw, W - x0)
        dst = out[b:b + 1] if b is not None else out
        dst[:, y0:y0 + rows, x0:x0 + cols] = seg[:rows, :cols, :].transpose(2, 0, 1)
    return out


# ---------------------------------------------------------------- the writer

def write_tiff(a, bigtiff=False, byteorder="<", tile=None, rows_per_strip=None, planar=2, predictor=1, compression=COMP_NONE,
               deflate_mode="dynamic", sample_format=1, extra_tags=(), segment_hook=None, packed=None, raw=None):
    """a: [C,H,W] uint8 / uint16.  The Predictor tag is written as given; the differencing is applied where libtiff applies
    it, with LZW and Deflate (its other codecs know no predictor: it writes the tag and stores the samples as they are, and
    ignores the tag when it reads).  Returns (file bytes, info) with info = dict(offsets, counts, raw) -- the segment table as
    written and the uncompressed segments.  segment_hook(index, compressed bytes) -> bytes lets a test damage a segment;
    `raw` / `packed` take segments prepared elsewhere (scripts/tiff_read_timing.py compresses a scene's on a thread pool)."""
    a = np.ascontiguousarray(a)
    C, H, W = a.shape
    bits = a.dtype.itemsize * 8
    applied = predictor if compression in (COMP_LZW, COMP_DEFLATE, COMP_DEFLATE_OLD) else 1      # as libtiff: see the docstring
    if raw is None:
        raw = raw_segments(a, tile, rows_per_strip, planar, applied, byteorder)
    spp_seg = C if planar == 1 else 1
    row_bytes = (tile[0] if tile else W) * spp_seg * a.dtype.itemsize
    if packed is None:
        packed = [compress(r, compression, deflate_mode, row_bytes) for r in raw]
    if segment_hook:
        packed = [bytes(segment_hook(i, p)) for i, p in enumerate(packed)]
    bo = byteorder
    head = 16 if bigtiff else 8
    offsets, at, body = [], head, bytearray()
    for p in packed:
        offsets.append(at)
        body += p
        if len(p) % 2:
            body += b"\0"
        at = head + len(body)
    counts = [len(p) for p in packed]
    LONGT = 16 if bigtiff else 4
    tags = [(256, 4, [W]), (257, 4, [H]), (258, 3, [bits] * C), (259, 3, [compression]), (262, 3, [1]), (277, 3, [C]),
            (284, 3, [planar]), (339, 3, [sample_format] * C)]
    if tile:
        tags += [(322, 4, [tile[0]]), (323, 4, [tile[1]]), (324, LONGT, offsets), (325, LONGT, counts)]
    else:
        tags += [(273, LONGT, offsets), (278, 4, [min(rows_per_strip or H, H)]), (279, LONGT, counts)]
    if predictor != 1:
        tags.append((317, 3, [predictor]))
    if C > 1:
        tags.append((338, 3, [0] * (C - 1)))
    tags += list(extra_tags)
    tags.sort(key=lambda t: t[0])
    fmt = {1: "B", 3: "H", 4: "I", 16: "Q"}
    ifd_at = at
    esize, inline = (20, 8) if bigtiff else (12, 4)
    extra_at = ifd_at + (8 if bigtiff else 2) + esize * len(tags) + (8 if bigtiff else 4)
    ifd = struct.pack(bo + ("Q" if bigtiff else "H"), len(tags))
    extra = bytearray()
    for tag, typ, vals in tags:
        data = struct.pack(bo + fmt[typ] * len(vals), *vals)
        if len(data) <= inline:
            field = data.ljust(inline, b"\0")
        else:
            field = struct.pack(bo + ("Q" if bigtiff else "I"), extra_at + len(extra))
            extra += data + (b"\0" if len(data) % 2 else b"")
        ifd += struct.pack(bo + "HH" + ("Q" if bigtiff else "I"), tag, typ, len(vals)) + field
    ifd += struct.pack(bo + ("Q" if bigtiff else "I"), 0)
    mark = b"II" if bo == "<" else b"MM"
    if bigtiff:
        header = mark + struct.pack(bo + "HHHQ", 43, 8, 0, ifd_at)
    else:
        header = mark + struct.pack(bo + "HI", 42, ifd_at)
    return bytes(header + body + ifd + extra), dict(offsets=offsets, counts=counts, raw=raw, predictor=applied)


# ---------------------------------------------------------------- a fixed list of damaged segments per codec

class _LsbWriter:
    """Deflate's bit order: fields from the least significant bit, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.nbits, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        self.acc |= value << self.nbits
        self.nbits += n
        while self.nbits >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.nbits -= 8

    def code(self, value, n):
        self.bits(int(format(value, f"0{n}b")[::-1], 2), n)

    def finish(self):
        if self.nbits:
            self.out.append(self.acc & 0xFF)
        return bytes(self.out)


def _fixed_literal(w, byte):
    if byte < 144:
        w.code(0x30 + byte, 8)
    else:
        w.code(0x190 + byte - 144, 9)


def lzw_codes(codes, width=9):
    w = _MsbWriter()
    for c in codes:
        w.put(c, width)
    return w.finish()


def damage_cases(compression, stream, expect):
    """[(name, bytes)]: about twenty damaged versions of `stream`, a sound segment of `expect` (> 300) uncompressed bytes in
    this compression.  Every one must end in a non-zero status: none of them yields `expect` bytes of a sound stream."""
    n = len(stream)
    # (an LZW stream ends in its last code and EOI, which a reader that stops at the expected size does not need: its late
    # cuts lie further in front of the end)
    late = (3 * n // 4, max(n - 8, 0)) if compression == COMP_LZW else (max(n - 5, 0), n - 1)
    cuts = sorted({0, 1, 2, 3, n // 4, n // 2} | set(late))
    cases = [(f"cut{k}", stream[:k]) for k in cuts]
    if compression in (COMP_DEFLATE, COMP_DEFLATE_OLD):
        body = stream[2:]
        cases += [("header-method", bytes([0x79, stream[1]]) + body),
                  ("header-check", bytes([stream[0], stream[1] ^ 1]) + body),
                  ("header-dictionary", bytes([0x78, 0x20]) + body),
                  ("header-window", bytes([0x88, 0x1C]) + body),
                  ("adler-last", stream[:-1] + bytes([stream[-1] ^ 0xFF])),
                  ("adler-first", stream[:-4] + bytes([stream[-4] ^ 1]) + stream[-3:])]
        w = _LsbWriter()      # a match that reaches before the segment's start: 'a', then length 3 at distance 2
        w.bits(1, 1); w.bits(1, 2); _fixed_literal(w, 97); w.code(1, 7); w.code(1, 5); w.code(0, 7)
        cases.append(("distance-before-start", b"\x78\x9c" + w.finish() + b"\0\0\0\0"))
        cases.append(("block-type-3", b"\x78\x9c\x07" + body))
        cases.append(("stored-length-mismatch", b"\x78\x9c\x01\x05\x00\xfa\xfe" + b"hello" + b"\0\0\0\0"))
        w = _LsbWriter()      # a dynamic block whose code length code is over-subscribed: nineteen lengths of 1
        w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
        for _ in range(19):
            w.bits(1, 3)
        cases.append(("oversubscribed-code", b"\x78\x9c" + w.finish() + b"\0" * 8))
        w = _LsbWriter()      # the fixed code's literal/length symbol 286, which no length uses
        w.bits(1, 1); w.bits(1, 2); _fixed_literal(w, 97); w.code(0xC6, 8)
        cases.append(("length-symbol-286", b"\x78\x9c" + w.finish() + b"\0" * 8))
        w = _LsbWriter()      # the fixed code's distance symbol 30
        w.bits(1, 1); w.bits(1, 2); _fixed_literal(w, 97); w.code(1, 7); w.code(30, 5)
        cases.append(("distance-symbol-30", b"\x78\x9c" + w.finish() + b"\0" * 8))
        w = _LsbWriter()      # a sound start, then the stream's end inside the block
        w.bits(0, 1); w.bits(1, 2)
        for c in b"abcabcabc":
            _fixed_literal(w, c)
        cases.append(("ends-inside-block", b"\x78\x9c" + w.finish()))
    elif compression == COMP_LZW:
        cases += [("code-beyond-table", lzw_codes([CLEAR, 97, 300])),
                  ("code-beyond-table-2", lzw_codes([CLEAR, 97, 98, 260])),
                  ("entry-after-clear", lzw_codes([CLEAR, 258])),
                  ("eoi-after-clear", lzw_codes([CLEAR, EOI])),
                  ("early-eoi", lzw_codes([CLEAR, 97, 98, EOI])),
                  ("only-clears", lzw_codes([CLEAR] * 9)),
                  ("no-clear-bad-first", lzw_codes([300, 97])),
                  ("self-code-then-end", lzw_codes([CLEAR, 97, 258, 259])),
                  ("ones-in-the-middle", stream[:n // 2] + b"\xff" * (n - n // 2)),
                  ("ones-after-start", stream[:3] + b"\xff" * (n - 3)),
                  ("zeros-tail", stream[:n // 3] + b"\0" * 4),
                  ("clear-then-nothing", lzw_codes([CLEAR, 97, 98, 99, CLEAR]))]
    elif compression == COMP_PACKBITS:
        cases += [("literal-past-stream", bytes([5, 1, 2])),
                  ("replicate-without-value", bytes([0xFE])),
                  ("literal-past-segment", (bytes([127]) + bytes(range(128))) * (expect // 128) + bytes([127]) + bytes(range(128))),
                  ("replicate-past-segment", bytes([0x81, 7]) * (expect // 128 + 1)),
                  ("only-no-ops", bytes([0x80]) * 10),
                  ("no-ops-then-short", bytes([0x80, 0x80, 3, 1, 2, 3, 4])),
                  ("short-replicate", bytes([0x81, 9])),
                  ("literal-header-only", bytes([127])),
                  ("half-then-literal-past-stream", stream[:n // 2] + bytes([100, 1])),
                  ("replicate-at-the-end", bytes([0xFF, 1] * 20 + [0xFD])),
                  ("empty-after-no-op", bytes([0x80])),
                  ("two-runs-then-end", bytes([0, 5, 0xFE, 6]))]
    return cases
