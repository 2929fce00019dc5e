"""TIFF scenes that raster_io's own reader refuses -- tiled, LZW / Deflate / PackBits compressed, predictor 2, BigTIFF --
parsed on the host and decompressed on the GPU: the ctypes binding of liblbdrn_tiff.so (include/lbdrn_tiff.h,
csrc/tiff.hip, csrc/tiff.inc).  Built by csrc/build.py beside liblbdrn_hip.so; LBDRN_TIFF_LIB names another file.

    parse(buf, ifd=0)          an IFD of a classic TIFF or BigTIFF, either byte order -> Scene (layout + segment table)
    read_ifds(buf)             the offsets of the IFD chain; overview_ifds(buf): the positions of the overview levels in it
    read_geo_tags(buf)         the GeoTIFF and GDAL tags of the first IFD, verbatim, for tiff_write's `geo`
    read_device(path, device)  contiguous [C,H,W] tensor in HBM: int16 storage for 16-bit samples, like every plane of this
                               package, uint8 for 8-bit ones
    read(path, device)         numpy, with the conventions of raster_io._read_tiff ([H,W] for one band)
    plan_window(scene, window) the segments a window (x0, y0, w, h) touches, as a scene of their own: sub-layout, byte ranges of the
                               file, the segment table rebased into the compact buffer of those ranges (host arithmetic)
    read_window_bytes(buf, path, window, device, ifd)   that window as a [C,h,w] tensor: only the touched segments are read,
                               uploaded and decoded; read_window(path, ...): the same over a read-only memory map -> numpy

A file is read through len() and slices only: bytes, a memory map or anything else that has them.
Everything outside the subset raises ValueError naming the tag and value before any device work.  Georeferencing tags are
never interpreted: read_geo_tags copies them for a writer to carry over."""
import ctypes
import struct
import zlib

import numpy as np

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
COMP_NONE, COMP_LZW, COMP_DEFLATE, COMP_DEFLATE_OLD, COMP_PACKBITS = 1, 5, 8, 32946, 32773
STATUS_TEXT = {1: "the stream ends before the segment is complete", 2: "invalid code", 3: "a match distance points before the segment",
               4: "bad zlib header", 5: "wrong Adler-32"}


class TiffError(NativeError):
    pass


class Layout(ctypes.Structure):
    """lbdrn_tiff_layout"""
    _fields_ = [(n, ctypes.c_int32) for n in ("C", "H", "W", "bits", "big_endian", "planar", "seg_w", "seg_h", "tiled",
                                              "compression", "predictor")]


_vp, _sz, _lp = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Layout)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_tiff.h
    "lbdrn_tiff_last_error": (ctypes.c_char_p, []),
    "lbdrn_tiff_abi_version": (ctypes.c_int, []),
    "lbdrn_tiff_segment_count": (_sz, [_lp]),
    "lbdrn_tiff_segment_cap": (_sz, [ctypes.c_int32]),
    "lbdrn_tiff_workspace": (_sz, [_lp]),
    "lbdrn_tiff_decode": (ctypes.c_int, [_lp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_tiff.so", "LBDRN_TIFF_LIB", "lbdrn_tiff_", ABI_VERSION, SIGNATURES, TiffError)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


# ---------------------------------------------------------------- the parser

# type -> (struct code, bytes); 16-18 are BigTIFF's LONG8, SLONG8, IFD8
_FIELD = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2), 9: ("i", 4),
          10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 13: ("I", 4), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
_WANTED = {254: "NewSubfileType", 256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 273: "StripOffsets",
           277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration", 317: "Predictor",
           322: "TileWidth", 323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 338: "ExtraSamples", 339: "SampleFormat"}


class Scene:
    """what parse() returns: the layout the library takes, the segment table, and the sample format for the host paths"""

    def __init__(self, layout, offsets, counts, sample_format, byteorder, names=None):
        self.layout, self.offsets, self.counts = layout, offsets, counts
        self.sample_format, self.byteorder = sample_format, byteorder
        self.names = names      # the sub-layout of a window: the file's own index of each segment, for the error messages

    @property
    def shape(self):
        return self.layout.C, self.layout.H, self.layout.W

    def plain_strips(self):
        """the subset raster_io._read_tiff reads by itself"""
        return self.layout.compression == COMP_NONE and not self.layout.tiled


def _unpack(fmt, buf, at):
    """struct.unpack_from through a slice: the parser reads a file through len() and slices only, so that a memory map is
    never copied whole and a wrapper that records its slices sees every byte that was touched"""
    return struct.unpack(fmt, buf[at:at + struct.calcsize(fmt)])


def _header(buf, path):
    """(byte order mark, BigTIFF?, offset of the first IFD)"""
    bo = {b"II": "<", b"MM": ">"}.get(bytes(buf[:2]))
    if bo is None or len(buf) < 8:
        raise ValueError(f"{path}: not a TIFF (no II / MM byte order mark)")
    magic = _unpack(bo + "H", buf, 2)[0]
    if magic == 42:
        return bo, False, _unpack(bo + "I", buf, 4)[0]
    if magic == 43:
        if len(buf) < 16 or _unpack(bo + "HH", buf, 4) != (8, 0):
            raise ValueError(f"{path}: BigTIFF header with an offset size other than 8")
        return bo, True, _unpack(bo + "Q", buf, 8)[0]
    raise ValueError(f"{path}: not a TIFF (magic {magic})")


MAX_IFDS = 4096      # the chain is walked no further: a pyramid has some twenty levels


def read_ifds(buf, path="TIFF"):
    """The offsets of the file's IFDs in chain order.  ValueError for an IFD or a next-IFD field outside the file, for a chain
    that comes back to an IFD it has visited, and for one longer than MAX_IFDS."""
    bo, big, off = _header(buf, path)
    cnt_fmt, cnt_size, ent, nxt_fmt, nxt_size = ("Q", 8, 20, "Q", 8) if big else ("H", 2, 12, "I", 4)
    out, seen = [], set()
    while off:
        if off in seen:
            raise ValueError(f"{path}: the IFD chain loops: IFD {len(out)} is at offset {off}, where an earlier one lies")
        if len(out) >= MAX_IFDS:
            raise ValueError(f"{path}: more than {MAX_IFDS} IFDs")
        if off + cnt_size > len(buf):
            raise ValueError(f"{path}: IFD {len(out)} (offset {off}) lies outside the file's {len(buf)} bytes")
        n = _unpack(bo + cnt_fmt, buf, off)[0]
        end = off + cnt_size + ent * n
        if end + nxt_size > len(buf):
            raise ValueError(f"{path}: IFD {len(out)} (offset {off}, {n} entries) lies outside the file's {len(buf)} bytes")
        seen.add(off)
        out.append(off)
        off = _unpack(bo + nxt_fmt, buf, end)[0]
    return out


def _ifd_offset(buf, path, ifd):
    """(byte order mark, BigTIFF?, offset of IFD number `ifd`, what to call it); ifd = 0 reads the header alone"""
    bo, big, off = _header(buf, path)
    if ifd == 0:
        return bo, big, off, "the first IFD"
    ifds = read_ifds(buf, path)
    if not 0 <= ifd < len(ifds):
        raise IndexError(f"{path}: IFD {ifd} of a file that has {len(ifds)}")
    return bo, big, ifds[ifd], f"IFD {ifd}"


def read_tags(buf, path="TIFF", ifd=0):
    """{tag: [values]} of the first IFD (or of IFD number `ifd` of the chain), the byte order mark ('<' or '>') and whether
    the file is a BigTIFF"""
    bo, big, off, name = _ifd_offset(buf, path, ifd)
    cnt_fmt, cnt_size, ent, inline = ("Q", 8, 20, 8) if big else ("H", 2, 12, 4)
    if off + cnt_size > len(buf):
        raise ValueError(f"{path}: {name} lies outside the file")
    n = _unpack(bo + cnt_fmt, buf, off)[0]
    if off + cnt_size + ent * n > len(buf):
        raise ValueError(f"{path}: {name} lies outside the file")
    tags = {}
    for i in range(n):
        at = off + cnt_size + ent * i
        tag, typ = _unpack(bo + "HH", buf, at)
        cnt = _unpack(bo + ("Q" if big else "I"), buf, at + 4)[0]
        if tag not in _WANTED or typ not in _FIELD:
            continue
        code, size = _FIELD[typ]
        if typ in (2, 5, 10, 11, 12):
            raise ValueError(f"{path}: tag {tag} ({_WANTED[tag]}) has the non-integer type {typ}")
        val_at = at + 4 + (8 if big else 4)
        if size * cnt > inline:
            val_at = _unpack(bo + ("Q" if big else "I"), buf, val_at)[0]
        if val_at + size * cnt > len(buf):
            raise ValueError(f"{path}: the values of tag {tag} ({_WANTED[tag]}) lie outside the file")
        tags[tag] = np.frombuffer(buf[val_at:val_at + size * cnt], np.dtype(bo + {"B": "u1", "b": "i1", "H": "u2", "h": "i2", "I": "u4",
                                                                                  "i": "i4", "Q": "u8", "q": "i8"}[code]),
                                  cnt).astype(np.int64 if code in "bhiq" else np.uint64).tolist()
    return tags, bo, big


def parse(buf, path="TIFF", ifd=0):
    """Scene of the first IFD, or of IFD number `ifd` of the chain (IndexError where the file has fewer); ValueError naming
    the tag and value for everything outside the subset."""
    return _parse(buf, path, ifd, True)


def _old_lzw(buf, path, offsets, counts, segments):
    """ValueError for a segment of `segments` that is old-style LZW, as libtiff detects the old bit order"""
    for i in segments:
        o, c = int(offsets[i]), int(counts[i])
        if c >= 2 and bytes(buf[o:o + 2]) in _OLD_LZW:
            raise ValueError(f"{path}: Compression (259) = 5: segment {i} is old-style (LSB-first) LZW, which is not read here")


_OLD_LZW = {bytes([0, b]) for b in range(1, 256, 2)}


def _parse(buf, path, ifd, lzw_check):
    """parse; lzw_check=False leaves the look at every LZW segment's first two bytes to the caller, who reads only some"""
    tags, bo, _ = read_tags(buf, path, ifd)

    def one(tag, default=None):
        v = tags.get(tag)
        if v is None:
            if default is None:
                raise ValueError(f"{path}: tag {tag} ({_WANTED[tag]}) is missing")
            return default
        return int(v[0])
    W, H = one(256), one(257)
    C = one(277, 1)
    bits = [int(b) for b in tags.get(258, [1])]
    if len(bits) == 1 and C > 1:
        bits = bits * C
    comp = one(259, 1)
    planar = one(284, 1)
    # libtiff knows the predictor with LZW and Deflate only: with PackBits or no compression it writes the tag and stores the
    # samples as they are, and ignores the tag when it reads.  So does this reader.
    pred = one(317, 1) if comp in (COMP_LZW, COMP_DEFLATE, COMP_DEFLATE_OLD) else 1
    fmt = [int(f) for f in tags.get(339, [1])]
    if len(set(bits)) != 1 or len(bits) != C:
        raise ValueError(f"{path}: BitsPerSample (258) = {bits}: mixed bit depths")
    if len(set(fmt)) != 1:
        raise ValueError(f"{path}: SampleFormat (339) = {fmt}: mixed sample formats")
    if comp not in (COMP_NONE, COMP_LZW, COMP_DEFLATE, COMP_DEFLATE_OLD, COMP_PACKBITS):
        raise ValueError(f"{path}: Compression (259) = {comp} is not read here (none, LZW 5, Deflate 8 / 32946, PackBits 32773 are)")
    if pred not in (1, 2):
        raise ValueError(f"{path}: Predictor (317) = {pred} is not read here (1 and 2 are)")
    if planar not in (1, 2):
        raise ValueError(f"{path}: PlanarConfiguration (284) = {planar}")
    if fmt[0] != 1:
        raise ValueError(f"{path}: SampleFormat (339) = {fmt[0]}: only unsigned integer samples are read from tiled or compressed files")
    if bits[0] not in (8, 16):
        raise ValueError(f"{path}: BitsPerSample (258) = {bits[0]}: only 8 and 16 bits are read from tiled or compressed files")
    if not (1 <= W <= 1 << 20 and 1 <= H <= 1 << 20 and 1 <= C <= 65535):
        raise ValueError(f"{path}: ImageWidth (256) x ImageLength (257) x SamplesPerPixel (277) = {W} x {H} x {C} is out of range")
    tiled = 322 in tags or 324 in tags
    if tiled:
        sw, sh = one(322), one(323)
        offsets, counts = tags.get(324), tags.get(325)
        names = "TileOffsets (324) / TileByteCounts (325)"
        if not (1 <= sw <= 1 << 20 and 1 <= sh <= 1 << 20):
            raise ValueError(f"{path}: TileWidth (322) x TileLength (323) = {sw} x {sh} is out of range")
    else:
        sw, sh = W, min(max(one(278, 0xFFFFFFFF), 1), H)
        offsets, counts = tags.get(273), tags.get(279)
        names = "StripOffsets (273) / StripByteCounts (279)"
    nseg = -(-W // sw) * -(-H // sh) * (C if planar == 2 else 1)
    if offsets is None or counts is None or len(offsets) != nseg or len(counts) != nseg:
        raise ValueError(f"{path}: {names}: {nseg} entries expected, {None if offsets is None else len(offsets)} / "
                         f"{None if counts is None else len(counts)} found")
    for i, (o, c) in enumerate(zip(offsets, counts)):
        if o + c > len(buf):
            raise ValueError(f"{path}: {names}: segment {i} (offset {o}, {c} bytes) lies outside the file's {len(buf)} bytes")
    if comp == COMP_LZW and lzw_check:
        _old_lzw(buf, path, offsets, counts, range(nseg))
    lay = Layout(C, H, W, bits[0], 1 if bo == ">" else 0, planar, sw, sh, 1 if tiled else 0,
                 COMP_DEFLATE if comp == COMP_DEFLATE_OLD else comp, pred)
    return Scene(lay, np.asarray(offsets, np.uint64), np.asarray(counts, np.uint64), fmt[0], bo)


# ---------------------------------------------------------------- overviews and georeferencing tags

def overview_ifds(buf, path="TIFF"):
    """the chain positions of the file's overview levels: the IFDs whose NewSubfileType (254) has bit 0 set, in file order"""
    out = []
    for i in range(len(read_ifds(buf, path))):
        if i and int(read_tags(buf, path, i)[0].get(254, [0])[0]) & 1:
            out.append(i)
    return out


# ModelPixelScale, ModelTiepoint, ModelTransformation (DOUBLE), GeoKeyDirectory (SHORT), GeoDoubleParams (DOUBLE),
# GeoAsciiParams, GDAL_METADATA, GDAL_NODATA (ASCII): tag -> (type, bytes of an element)
GEO_TAGS = {33550: (12, 8), 33922: (12, 8), 34264: (12, 8), 34735: (3, 2), 34736: (12, 8), 34737: (2, 1), 42112: (2, 1), 42113: (2, 1)}


def read_geo_tags(buf, path="TIFF"):
    """The georeferencing tags of the first IFD as [(tag, type, count, value bytes)], the values little-endian whatever the
    file's byte order: copied, never interpreted.  [] for a file that has none.  What tiff_write takes as `geo`."""
    bo, big, off, name = _ifd_offset(buf, path, 0)
    cnt_fmt, cnt_size, ent, inline = ("Q", 8, 20, 8) if big else ("H", 2, 12, 4)
    if off + cnt_size > len(buf):
        raise ValueError(f"{path}: {name} lies outside the file")
    n = _unpack(bo + cnt_fmt, buf, off)[0]
    if off + cnt_size + ent * n > len(buf):
        raise ValueError(f"{path}: {name} lies outside the file")
    out = []
    for i in range(n):
        at = off + cnt_size + ent * i
        tag, typ = _unpack(bo + "HH", buf, at)
        if tag not in GEO_TAGS or typ != GEO_TAGS[tag][0]:
            continue
        cnt = _unpack(bo + ("Q" if big else "I"), buf, at + 4)[0]
        size = GEO_TAGS[tag][1]
        val_at = at + 4 + (8 if big else 4)
        if size * cnt > inline:
            val_at = _unpack(bo + ("Q" if big else "I"), buf, val_at)[0]
        if val_at + size * cnt > len(buf):
            raise ValueError(f"{path}: the values of tag {tag} lie outside the file")
        raw = np.frombuffer(buf[val_at:val_at + size * cnt], np.dtype(bo + "u%d" % size), cnt).astype("<u%d" % size).tobytes()
        out.append((int(tag), int(typ), int(cnt), raw))
    return out


# ---------------------------------------------------------------- the host path of an oversize Deflate segment

def _segment_grid(lay):
    per_row = -(-lay.W // lay.seg_w)
    rows = -(-lay.H // lay.seg_h)
    for b in (range(lay.C) if lay.planar == 2 else [None]):
        for ty in range(rows):
            for tx in range(per_row):
                yield b, ty * lay.seg_h, tx * lay.seg_w


def _name(scene, i):
    """what an error calls segment i of the scene: its index in the file's own table"""
    return i if scene.names is None else int(scene.names[i])


def _read_host_deflate(buf, scene):
    """zlib on the host, un-predicted and placed in numpy like raster_io's own reader: for a Deflate file whose writer put more
    into one segment than the device decodes (a whole band in one strip)"""
    lay = scene.layout
    dt = np.dtype(scene.byteorder + ("u1" if lay.bits == 8 else "u2"))
    native = dt.newbyteorder("=")
    out = np.zeros((lay.C, lay.H, lay.W), native)
    spp = 1 if lay.planar == 2 else lay.C
    for i, (b, y0, x0) in enumerate(_segment_grid(lay)):
        rows = min(lay.seg_h, lay.H - y0)
        hh = lay.seg_h if lay.tiled else rows
        o, c = int(scene.offsets[i]), int(scene.counts[i])
        try:
            raw = zlib.decompress(bytes(buf[o:o + c]))
        except zlib.error as e:
            raise TiffError(f"segment {_name(scene, i)} is damaged: {e}") from None
        if len(raw) < hh * lay.seg_w * spp * dt.itemsize:
            raise TiffError(f"segment {_name(scene, i)} is damaged: it holds {len(raw)} bytes of {hh * lay.seg_w * spp * dt.itemsize}")
        seg = np.frombuffer(raw, dt, hh * lay.seg_w * spp).astype(native).reshape(hh, lay.seg_w, spp)
        if lay.predictor == 2:
            seg = np.cumsum(seg, axis=1, dtype=native)
        cols = min(lay.seg_w, lay.W - x0)
        dst = out[b:b + 1] if b is not None else out
        dst[:, y0:y0 + rows, x0:x0 + cols] = seg[:rows, :cols, :].transpose(2, 0, 1)
    return out


def _segment_bytes(lay):
    return lay.seg_w * lay.seg_h * (1 if lay.planar == 2 else lay.C) * (lay.bits // 8)


def _over_cap(lay, path):
    """None, 'host' (Deflate: the interpreter's zlib takes it) or a ValueError for a layout whose segments are above the cap"""
    cap = lib().lbdrn_tiff_segment_cap(lay.compression)
    if _segment_bytes(lay) <= cap:
        return None
    if lay.compression == COMP_DEFLATE:
        return "host"
    raise ValueError(f"{path}: a segment of {_segment_bytes(lay)} bytes is above the cap of {cap} bytes the device decodes for "
                     f"Compression (259) = {lay.compression}, and there is no host decoder for it")


# ---------------------------------------------------------------- entry points

def _device(device):
    import torch
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise TiffError("a tiled or compressed TIFF is decompressed on the GPU; there is no CPU path in this package")
    return dev


def decode_device(buf, scene, dev):
    """the planes of a parsed scene as a [C,H,W] tensor on dev; buf: the file's bytes"""
    import torch
    lay = scene.layout
    L = lib()
    nseg = L.lbdrn_tiff_segment_count(ctypes.byref(lay))
    nws = L.lbdrn_tiff_workspace(ctypes.byref(lay))
    if not nseg or nseg != len(scene.offsets):
        raise TiffError("the layout is out of the library's range")
    offsets = np.ascontiguousarray(scene.offsets, np.uint64)
    counts = np.ascontiguousarray(scene.counts, np.uint64)
    with torch.cuda.device(dev):
        # the file is uploaded once (a window's compact buffer is a bytearray already)
        raw = torch.frombuffer(buf if isinstance(buf, bytearray) else bytearray(buf), dtype=torch.uint8).to(dev)
        planes = torch.empty((lay.C, lay.H, lay.W), dtype=torch.uint8 if lay.bits == 8 else torch.int16, device=dev)
        status = torch.empty(nseg, dtype=torch.int32, device=dev)
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        _check(L.lbdrn_tiff_decode(ctypes.byref(lay), raw.data_ptr(), raw.numel(), offsets.ctypes.data, counts.ctypes.data, nseg,
                                   planes.data_ptr(), status.data_ptr(), ws.data_ptr(), nws,
                                   torch.cuda.current_stream(dev).cuda_stream), "lbdrn_tiff_decode")
        st = status.cpu().numpy()      # the one host sync; offsets and counts have been copied by now
    bad = np.flatnonzero(st)
    if bad.size:
        i = int(bad[0])
        raise TiffError(f"segment {_name(scene, i)} is damaged: {STATUS_TEXT.get(int(st[i]), st[i])}" +
                        (f" ({bad.size} damaged segments in all)" if bad.size > 1 else ""), int(st[i]))
    return planes


def read_device(path, device=None):
    """contiguous [C,H,W] tensor in HBM: int16 storage for 16-bit samples, uint8 for 8-bit ones"""
    with open(path, "rb") as f:
        return read_device_bytes(f.read(), path, device)


def read_device_bytes(buf, path, device=None, ifd=0):
    """read_device of a file whose bytes the caller holds already; ifd: the IFD of the chain to read"""
    import torch
    scene = parse(buf, path, ifd)
    route = _over_cap(scene.layout, path)
    dev = _device(device)
    if route == "host":
        a = _read_host_deflate(buf, scene)
        t = torch.from_numpy(a.view(np.int16) if a.dtype.itemsize == 2 else a)
        return t.to(dev)
    return decode_device(buf, scene, dev)


def read(path, device=None, ifd=0):
    """numpy uint8 / uint16 [C,H,W], [H,W] for one band: what raster_io._read_tiff returns for the files it reads itself"""
    with open(path, "rb") as f:
        buf = f.read()
    scene = parse(buf, path, ifd)
    if _over_cap(scene.layout, path) == "host":
        a = _read_host_deflate(buf, scene)
    else:
        t = decode_device(buf, scene, _device(device)).cpu().numpy()
        a = t.view(np.uint16) if t.dtype == np.int16 else t
    return a[0] if a.shape[0] == 1 else a


# ---------------------------------------------------------------- a window of a scene

class WindowPlan:
    """What plan_window returns: the segments a window touches and how to hand them to the library as a scene of their own.

        segments  indices into the file's segment table, in the order the sub-layout wants them (TIFF order over the
                  covered sub-grid; planar = 2: all of band 0, then band 1, ...)
        layout    the Layout of the covered grid alone: [C, H', W']
        ranges    the (offset, length) byte ranges of the file that hold those segments, sorted, neighbours merged
        offsets, counts   the segment table rebased into the compact buffer made of `ranges` one after another
        crop      (oy, ox): where the window starts inside the cover
        nbytes    the length of the compact buffer"""

    def __init__(self, window, segments, layout, ranges, offsets, counts, crop):
        self.window, self.segments, self.layout, self.ranges = window, segments, layout, ranges
        self.offsets, self.counts, self.crop = offsets, counts, crop
        self.nbytes = sum(n for _, n in ranges)

    def gather(self, buf):
        """the compact buffer: `ranges` of buf one after another (never empty: the library takes no null pointer)"""
        out, at = bytearray(max(self.nbytes, 1)), 0
        for o, n in self.ranges:
            out[at:at + n] = buf[o:o + n]
            at += n
        return out


def plan_window(scene, window):
    """The plan of reading window = (x0, y0, w, h) of a parsed Scene: host arithmetic on the segment table, no byte of the
    file is looked at.  The window is checked as codec.check_window checks one."""
    from .codec import check_window
    lay = scene.layout
    x0, y0, w, h = check_window(window, lay.W, lay.H)
    sw, sh = lay.seg_w, lay.seg_h
    per_row, rows = -(-lay.W // sw), -(-lay.H // sh)
    tx0, tx1 = (x0 // sw, -(-(x0 + w) // sw)) if lay.tiled else (0, 1)      # strips: full rows
    ty0, ty1 = y0 // sh, -(-(y0 + h) // sh)
    Wc = min(tx1 * sw, lay.W) - tx0 * sw
    Hc = min(ty1 * sh, lay.H) - ty0 * sh
    sub = Layout(lay.C, Hc, Wc, lay.bits, lay.big_endian, lay.planar, sw, sh if lay.tiled else min(sh, Hc), lay.tiled,
                 lay.compression, lay.predictor)
    segments = [b * per_row * rows + ty * per_row + tx for b in range(lay.C if lay.planar == 2 else 1)
                for ty in range(ty0, ty1) for tx in range(tx0, tx1)]
    offs = [int(scene.offsets[i]) for i in segments]
    cnts = [int(scene.counts[i]) for i in segments]
    ranges = []      # [offset, end), sorted and merged where one begins at or before the end of the one in front of it
    for o, c in sorted((o, c) for o, c in zip(offs, cnts) if c):
        if ranges and o <= ranges[-1][1]:
            ranges[-1][1] = max(ranges[-1][1], o + c)
        else:
            ranges.append([o, o + c])
    starts = [r[0] for r in ranges]
    base = np.concatenate([[0], np.cumsum([r[1] - r[0] for r in ranges])]).astype(np.int64) if ranges else np.zeros(1, np.int64)
    rebased = []
    for o, c in zip(offs, cnts):
        k = int(np.searchsorted(starts, o, side="right")) - 1 if c else -1
        rebased.append(int(base[k]) + o - starts[k] if c else 0)
    return WindowPlan((x0, y0, w, h), segments, sub, [(a, b - a) for a, b in ranges], np.asarray(rebased, np.uint64),
                      np.asarray(cnts, np.uint64), (y0 - ty0 * sh, x0 - tx0 * sw))


def _window_plain(buf, scene, plan):
    """The window of an uncompressed strip file, on the host: of every touched strip only the window's rows are read, then
    the columns are sliced -> numpy [C,h,w]"""
    lay = scene.layout
    x0, y0, w, h = plan.window
    dt = np.dtype(scene.byteorder + ("u1" if lay.bits == 8 else "u2"))
    spp = 1 if lay.planar == 2 else lay.C
    row_bytes = lay.W * spp * dt.itemsize
    rows_y = -(-lay.H // lay.seg_h)
    out = np.empty((lay.C, h, w), dt.newbyteorder("="))
    for i in plan.segments:
        b, ty = divmod(i, rows_y)
        s0 = ty * lay.seg_h
        r0, r1 = max(y0, s0), min(y0 + h, s0 + lay.seg_h, lay.H)
        o, c = int(scene.offsets[i]), int(scene.counts[i])
        if c < (min(lay.seg_h, lay.H - s0)) * row_bytes:
            raise TiffError(f"segment {i} is damaged: {STATUS_TEXT[1]}", 1)
        raw = buf[o + (r0 - s0) * row_bytes:o + (r1 - s0) * row_bytes]
        part = np.frombuffer(raw, dt, (r1 - r0) * lay.W * spp).reshape(r1 - r0, lay.W, spp)[:, x0:x0 + w, :]
        dst = out[b:b + 1] if lay.planar == 2 else out
        dst[:, r0 - y0:r1 - y0, :] = part.transpose(2, 0, 1)
    return out


def _window(buf, path, window, device, ifd, tensor):
    """read_window_bytes (tensor=True) and read_window (False): a host route leaves the device alone where numpy is asked for"""
    import torch
    scene = _parse(buf, path, ifd, False)
    plan = plan_window(scene, window)
    lay = plan.layout
    if lay.compression == COMP_LZW:
        _old_lzw(buf, path, scene.offsets, scene.counts, plan.segments)
    (oy, ox), (_, _, w, h) = plan.crop, plan.window
    a = None
    if scene.plain_strips():
        a = _window_plain(buf, scene, plan)
    else:
        route = _over_cap(lay, path)
        sub = Scene(lay, plan.offsets, plan.counts, scene.sample_format, scene.byteorder, names=plan.segments)
        if route == "host":
            a = np.ascontiguousarray(_read_host_deflate(plan.gather(buf), sub)[:, oy:oy + h, ox:ox + w])
    if a is not None:
        if not tensor:
            return a
        return torch.from_numpy(a.view(np.int16) if a.dtype.itemsize == 2 else a).to(_device(device))
    t = decode_device(plan.gather(buf), sub, _device(device))[:, oy:oy + h, ox:ox + w].contiguous()
    if tensor:
        return t
    t = t.cpu().numpy()
    return t.view(np.uint16) if t.dtype == np.int16 else t


def read_window_bytes(buf, path, window, device=None, ifd=0):
    """window = (x0, y0, w, h) of IFD `ifd` as a contiguous [C,h,w] tensor on the device, bit for bit that slice of
    read_device_bytes.  buf: the file as anything that has len() and slices -- bytes, a memory map.  Only the header, the
    IFD chain, the tag arrays and the segments the window touches are read; those segments alone are uploaded, as one
    compact buffer, and decoded as a scene of their own (plan_window).  A damaged segment elsewhere is never looked at;
    one inside raises TiffError under its index in the file."""
    return _window(buf, path, window, device, ifd, True)


def open_map(path):
    """the file as a read-only memory map (an empty file: its no bytes, which the parser refuses by name)"""
    import mmap
    with open(path, "rb") as f:
        try:
            return mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            return f.read()


def read_window(path, window, device=None, ifd=0):
    """read_window_bytes of a file opened as a read-only memory map -> numpy uint8 / uint16 [C,h,w].  An uncompressed strip
    file and an over-cap Deflate one never touch the device."""
    buf = open_map(path)
    try:
        return _window(buf, path, window, device, ifd, False)
    finally:
        if not isinstance(buf, bytes):
            buf.close()
