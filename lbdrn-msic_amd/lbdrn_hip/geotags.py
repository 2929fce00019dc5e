"""A scene's georeferencing and nodata tags as data: the trailer chunk that carries them through a .bin, and their move
under a crop.  Host code only: nothing here touches the device.

The tag list is what tiff.read_geo_tags returns and tiff_write takes as `geo`: [(tag, type, count, little-endian value
bytes)] over the eight tags of tiff.GEO_TAGS.

    pack(tags) -> bytes, unpack(bytes) -> tags      one trailer chunk, 'LBGT' (big-endian framing, like the header and 'LBRT'):

        'L' 'B' 'G' 'T' | version u8 = 1 | flags u8 | reserved u16 = 0 | payload bytes u32 | payload | CRC-32 u32

      flags bit 0: the payload is a zlib stream (zlib.compress(raw, 9)), set exactly when that stream is shorter than raw;
      every other bit is 0.  The CRC is zlib.crc32 of the uncompressed payload.
        raw = count u16, then per tag, in ascending tag order:  tag u16 | type u16 | count u32 | value bytes
      (these fields big-endian too; the value bytes are read_geo_tags', unchanged).  The bytes are a function of the tag
      list alone.  container.pack_geo_trailer / unpack_geo_trailer place the chunk in a file.

    shift(tags, x0, y0) -> tags      the tags of the crop whose pixel (0, 0) is the scene's pixel (x0, y0).  IEEE float64, in
      exactly the order written here:
        ModelTiepoint (33922) of exactly 6 doubles (I, J, K, X, Y, Z) beside a ModelPixelScale (33550) (Sx, Sy, Sz):
            X' = X + x0 * Sx,  Y' = Y - y0 * Sy;  I, J, K, Z unchanged -- the numbers a `gdal_translate -srcwin` crop carries
        any other ModelTiepoint (several tiepoints, or no pixel scale): for every tiepoint I' = I - x0, J' = J - y0 (exact);
            the model coordinates are unchanged
        ModelTransformation (34264: 16 doubles, row-major M, model = M (i, j, k, 1)):
            for r in 0..2:  M'[r][3] = (M[r][3] + M[r][0] * x0) + M[r][1] * y0;  the rest unchanged
      A file that has both 33922 and 34264 gets each tag's own rule.  Everything else -- ModelPixelScale, the GeoKey tags,
      GDAL_METADATA, GDAL_NODATA -- is carried verbatim.  NOT moved: the RPC offsets (LINE_OFF, SAMP_OFF) inside a
      GDAL_METADATA item; a crop of an RPC-referenced scene keeps the scene's coefficients.  shift(tags, 0, 0) returns the
      tags byte for byte.

    python -m lbdrn_hip.geotags FILE.tif | FILE.bin                                       the tags, one line per tag
    python -m lbdrn_hip.geotags --attach SCENE.tif FILE.bin [-o OUT.bin] [--window X0 Y0 W H]
                                             append the chunk to an encoded file -- the bytes encode.py --keep-tags writes
    python -m lbdrn_hip.geotags --strip FILE.bin [-o OUT.bin]                              remove it
"""
import struct
import zlib

from .tiff import GEO_TAGS

MAGIC = b"LBGT"
VERSION = 1
FLAG_ZLIB = 0x01
MAX_RAW = 1 << 26      # what unpack will inflate a payload to: GDAL_METADATA with RPCs is kilobytes

PIXEL_SCALE, TIEPOINT, TRANSFORMATION, GDAL_NODATA = 33550, 33922, 34264, 42113
NAMES = {33550: "ModelPixelScale", 33922: "ModelTiepoint", 34264: "ModelTransformation", 34735: "GeoKeyDirectory",
         34736: "GeoDoubleParams", 34737: "GeoAsciiParams", 42112: "GDAL_METADATA", 42113: "GDAL_NODATA"}


def _checked(tags):
    """the tag list as [(int, int, int, bytes)] in ascending tag order; ValueError for a list no chunk carries"""
    out, seen = [], set()
    for item in tags:
        try:
            tag, typ, cnt, raw = item
            tag, typ, cnt, raw = int(tag), int(typ), int(cnt), bytes(raw)
        except (TypeError, ValueError):
            raise ValueError(f"geo tags: {item!r} is no (tag, type, count, value bytes)") from None
        if tag not in GEO_TAGS:
            raise ValueError(f"geo tags: tag {tag} is none of {sorted(GEO_TAGS)}")
        if typ != GEO_TAGS[tag][0]:
            raise ValueError(f"geo tags: tag {tag} has type {typ}, {NAMES[tag]} is of type {GEO_TAGS[tag][0]}")
        if tag in seen:
            raise ValueError(f"geo tags: tag {tag} is given twice")
        if not 1 <= cnt < 1 << 32 or len(raw) != cnt * GEO_TAGS[tag][1]:
            raise ValueError(f"geo tags: tag {tag}: {len(raw)} value bytes for {cnt} values of {GEO_TAGS[tag][1]} bytes")
        seen.add(tag)
        out.append((tag, typ, cnt, raw))
    out.sort(key=lambda t: t[0])
    return out


def pack(tags):
    """The 'LBGT' chunk of a tag list (the module's docstring has the layout).  ValueError for a tag outside GEO_TAGS, a type
    other than the tag's, a tag given twice and a value whose length is not count x element size."""
    tags = _checked(tags)
    raw = struct.pack(">H", len(tags)) + b"".join(struct.pack(">HHI", tag, typ, cnt) + val for tag, typ, cnt, val in tags)
    packed = zlib.compress(raw, 9)
    flags, payload = (FLAG_ZLIB, packed) if len(packed) < len(raw) else (0, raw)
    if len(payload) >= 1 << 32:
        raise OverflowError(f"geo tags: a payload of {len(payload)} bytes does not fit its 4-byte size field")
    return MAGIC + struct.pack(">BBHI", VERSION, flags, 0, len(payload)) + payload + struct.pack(">I", zlib.crc32(raw))


def unpack(buf):
    """The tag list of one 'LBGT' chunk -- `buf` is the chunk and nothing else.  ValueError for another magic, a newer
    version, a non-zero reserved field, an unknown flag, a size that does not fill `buf`, a zlib error, a CRC mismatch, tags
    out of order, and for any list pack() would have refused: what comes back can always be packed again."""
    buf = bytes(buf)
    if len(buf) < 16 or buf[:4] != MAGIC:
        raise ValueError(f"{len(buf)} bytes that are no geo-tag chunk ('LBGT')")
    version, flags, reserved, n = struct.unpack_from(">BBHI", buf, 4)
    if version != VERSION:
        raise ValueError(f"geo-tag chunk version {version}: written by a newer version of this package")
    if reserved or flags & ~FLAG_ZLIB:
        raise ValueError(f"geo-tag chunk with flags {flags:#x} / reserved field {reserved:#x}: written by a newer version of this package")
    if 12 + n + 4 != len(buf):
        raise ValueError(f"geo-tag chunk lists a payload of {n} bytes, {len(buf) - 16} are there")
    raw = buf[12:12 + n]
    if flags & FLAG_ZLIB:
        try:
            z = zlib.decompressobj()
            raw = z.decompress(raw, MAX_RAW)
            if z.unconsumed_tail or not z.eof or z.unused_data:
                raise ValueError("geo-tag chunk: the zlib stream does not end where the payload ends, or inflates past "
                                 f"{MAX_RAW} bytes")
        except zlib.error as e:
            raise ValueError(f"geo-tag chunk: {e}") from None
        if n >= len(raw):
            raise ValueError("geo-tag chunk: a compressed payload that is no shorter than what it holds")
    if zlib.crc32(raw) != struct.unpack_from(">I", buf, 12 + n)[0]:
        raise ValueError("geo-tag chunk: CRC mismatch")
    if len(raw) < 2:
        raise ValueError("geo-tag chunk: a payload without a tag count")
    count, pos, tags = struct.unpack_from(">H", raw, 0)[0], 2, []
    for _ in range(count):
        if pos + 8 > len(raw):
            raise ValueError("geo-tag chunk: the payload ends inside a tag")
        tag, typ, cnt = struct.unpack_from(">HHI", raw, pos)
        if tags and tag <= tags[-1][0]:
            raise ValueError(f"geo-tag chunk: tag {tag} behind tag {tags[-1][0]}: out of order")
        size = cnt * GEO_TAGS.get(tag, (0, 1))[1]
        if pos + 8 + size > len(raw):
            raise ValueError(f"geo-tag chunk: the values of tag {tag} end behind the payload")
        tags.append((tag, typ, cnt, raw[pos + 8:pos + 8 + size]))
        pos += 8 + size
    if pos != len(raw):
        raise ValueError(f"geo-tag chunk: {len(raw) - pos} payload bytes behind the last tag")
    return _checked(tags)


def _doubles(raw):
    return list(struct.unpack("<%dd" % (len(raw) // 8), raw))


def shift(tags, x0, y0):
    """The tags of the crop whose pixel (0, 0) is the scene's pixel (x0, y0): the three rules of the module's docstring, in
    float64 and in the order written there; every other tag verbatim; (0, 0) returns the tags byte for byte.  The RPC
    offsets inside GDAL_METADATA are not moved."""
    tags = [(int(tag), int(typ), int(cnt), bytes(raw)) for tag, typ, cnt, raw in tags]
    if x0 == 0 and y0 == 0:
        return tags
    scale = next((_doubles(raw) for tag, _, cnt, raw in tags if tag == PIXEL_SCALE and cnt == 3 and len(raw) == 24), None)
    out = []
    for tag, typ, cnt, raw in tags:
        if tag == TIEPOINT and len(raw) == 8 * cnt and cnt == 6 and scale is not None:
            I, J, K, X, Y, Z = _doubles(raw)
            raw = struct.pack("<6d", I, J, K, X + x0 * scale[0], Y - y0 * scale[1], Z)
        elif tag == TIEPOINT and len(raw) == 8 * cnt and cnt % 6 == 0:
            v = _doubles(raw)
            for k in range(0, cnt, 6):
                v[k], v[k + 1] = v[k] - x0, v[k + 1] - y0
            raw = struct.pack("<%dd" % cnt, *v)
        elif tag == TRANSFORMATION and len(raw) == 8 * cnt and cnt == 16:
            m = _doubles(raw)
            for r in range(3):
                m[4 * r + 3] = (m[4 * r + 3] + m[4 * r] * x0) + m[4 * r + 1] * y0
            raw = struct.pack("<16d", *m)
        out.append((tag, typ, cnt, raw))
    return out


def stored_nodata(tags, bits):
    """The value a GDAL_NODATA tag names, where it parses as an integer within the range of `bits`-bit samples; else None."""
    for tag, _, _, raw in tags or ():
        if tag == GDAL_NODATA:
            text = bytes(raw).split(b"\0")[0].decode("ascii", "replace").strip()
            if text and (text.isdigit() or (text[0] in "+-" and text[1:].isdigit())) and 0 <= int(text) < 1 << bits:
                return int(text)
    return None


def describe(tags):
    """One line per tag: number, name, count and the values (text for the ASCII tags, shortened where long)."""
    lines = []
    for tag, typ, cnt, raw in tags:
        if typ == 2:
            text = repr(bytes(raw).rstrip(b"\0").decode("ascii", "replace"))
            text = text if len(text) <= 100 else text[:97] + "..."
        else:
            vals = struct.unpack("<%d%s" % (cnt, "d" if typ == 12 else "H"), raw)
            text = " ".join(repr(v) for v in vals[:16]) + (" ..." if cnt > 16 else "")
        lines.append(f"{tag} {NAMES.get(tag, '?')} ({cnt}): {text}")
    return lines


def _cli(argv=None):
    import argparse
    from . import container, raster_io
    p = argparse.ArgumentParser(prog="python -m lbdrn_hip.geotags", description="the georeferencing tags of a TIFF or a .bin")
    p.add_argument("file", nargs="?", help="FILE.tif or FILE.bin: print its tags")
    p.add_argument("--attach", nargs=2, metavar=("SCENE.tif", "FILE.bin"), help="append SCENE's tags to FILE.bin")
    p.add_argument("--strip", metavar="FILE.bin", help="remove the tags from FILE.bin")
    p.add_argument("-o", dest="out", default=None, metavar="OUT.bin", help="with --attach / --strip: write here (default: in place)")
    p.add_argument("--window", type=int, nargs=4, default=None, metavar=("X0", "Y0", "W", "H"),
                   help="with --attach: FILE.bin holds this part of SCENE (encode.py --window)")
    a = p.parse_args(argv)
    if (a.file is not None) + (a.attach is not None) + (a.strip is not None) != 1:
        p.error("one of FILE, --attach SCENE.tif FILE.bin, --strip FILE.bin")
    if a.window is not None and a.attach is None:
        p.error("--window goes with --attach")
    if a.out is not None and a.file is not None:
        p.error("-o goes with --attach and --strip")
    if a.file is not None:
        if a.file.endswith(".bin"):
            with open(a.file, "rb") as f:
                tags = container.unpack_geo_trailer(f.read())
        else:
            tags = raster_io.read_geo_tags(a.file)
        for line in describe(tags or []):
            print(line)
        if not tags:
            print("no tags")
        return 0
    path = a.attach[1] if a.attach is not None else a.strip
    with open(path, "rb") as f:
        buf = f.read()
    if a.attach is not None:
        if container.unpack_geo_trailer(buf) is not None:
            p.error(f"{path} already carries tags (--strip removes them)")
        tags = raster_io.read_geo_tags(a.attach[0])
        _, h, w, _ = raster_io.raster_shape(a.attach[0])
        if a.window is not None:
            from .codec import check_window
            try:
                x0, y0, w, h = check_window(a.window, w, h)
            except ValueError as e:
                p.error(f"--window: {e}")
            tags = shift(tags, x0, y0)
        if (w, h) != tuple(container.unpack_header(buf)[2:4]):
            p.error("{} holds {} x {} pixels, {} has {} x {}".format(path, *container.unpack_header(buf)[2:4],
                                                                     "the window" if a.window is not None else a.attach[0], w, h))
        out = buf + (container.pack_geo_trailer(tags) if tags else b"")
        print(f"Tags: {len(tags)} tags, {len(out) - len(buf)} bytes" if tags else "Tags: none")
    else:
        out = container.strip_geo_trailer(buf)
    with open(a.out or path, "wb") as f:
        f.write(out)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(_cli())
