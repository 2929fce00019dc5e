"""Tiled or stripped, Deflate-compressed TIFF rasters written from planes in HBM: the ctypes binding of liblbdrn_tiffw.so
(include/lbdrn_tiff_write.h, csrc/tiffw.hip, csrc/tiffw.inc) and the container around the segments it returns.  Built by
csrc/build.py beside liblbdrn_tiff.so; LBDRN_TIFFW_LIB names another file.

    write_device(path, tensor, ...)  a [C,H,W] tensor in HBM (int16 storage for 16-bit samples, uint8 for 8-bit ones): the
                                     segments are gathered, predicted and Deflate-coded on the device; only the coded bytes
                                     and their table come to the host
    write(path, array, ...)          numpy uint8 / uint16 [C,H,W] or [H,W]: uploaded, then the same
    encode_device(tensor, layout)    the device stage alone -> (body bytes, offsets, counts)
    assemble(layout, counts)         the container alone -> (head bytes, offsets of the segments in the file)

The file is little-endian, classic TIFF, or BigTIFF when any offset would pass 2^32 - 1; it carries the tags
raster_io._write_tiff writes, plus Compression, Predictor (only when 2), PlanarConfiguration and the tile or strip tables;
three or more 8-bit bands are tagged RGB, the rest extra samples, as GDAL's GTiff driver tags them.

    write_device(..., overviews="auto" | N, resampling=, nodata=, geo=)   the overview levels reduced on the device by
                                     lbdrn_hip.pyramid and written as further IFDs; georeferencing tags copied onto the first
    assemble_pyramid(layouts, counts_per_level, geo)   the container of such a file

With neither overviews nor geo a file is byte for byte what it was before these options existed."""
import ctypes
import struct

import numpy as np

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
COMP_NONE, COMP_DEFLATE = 1, 8
DEFAULT_TILE = 256


class TiffWriteError(NativeError):
    pass


class Layout(ctypes.Structure):
    """lbdrn_tiffw_layout"""
    _fields_ = [(n, ctypes.c_int32) for n in ("C", "H", "W", "bits", "big_endian", "planar", "seg_w", "seg_h", "tiled",
                                              "compression", "predictor")]


_vp, _sz, _lp = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Layout)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_tiff_write.h
    "lbdrn_tiffw_last_error": (ctypes.c_char_p, []),
    "lbdrn_tiffw_abi_version": (ctypes.c_int, []),
    "lbdrn_tiffw_segment_count": (_sz, [_lp]),
    "lbdrn_tiffw_segment_cap": (_sz, [ctypes.c_int32]),
    "lbdrn_tiffw_bound": (_sz, [_sz]),
    "lbdrn_tiffw_block_tokens": (_sz, []),
    "lbdrn_tiffw_output_bytes": (_sz, [_lp]),
    "lbdrn_tiffw_workspace": (_sz, [_lp]),
    "lbdrn_tiffw_encode": (ctypes.c_int, [_lp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_tiffw.so", "LBDRN_TIFFW_LIB", "lbdrn_tiffw_", ABI_VERSION, SIGNATURES, TiffWriteError)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


# ---------------------------------------------------------------- the layout of a call

def segment_count(lay):
    """the segments of a layout, from its fields alone"""
    return -(-lay.W // lay.seg_w) * -(-lay.H // lay.seg_h) * (lay.C if lay.planar == 2 else 1)


def segment_bytes(lay):
    return lay.seg_w * lay.seg_h * (1 if lay.planar == 2 else lay.C) * (lay.bits // 8)


def make_layout(C, H, W, bits, compress=None, tile=None, rows_per_strip=None, planar=2, predictor=None, cap=None):
    """The Layout of a write: compress None / "none" / "deflate"; tile None, N or (tile_w, tile_h); rows_per_strip for strips
    instead.  Defaults: 256 x 256 tiles, planar, predictor 2 with Deflate.  ValueError for what the format or the library
    does not take; cap: the segment cap to hold the layout to (default: the library's)."""
    if compress in (None, "none"):
        comp = COMP_NONE
    elif compress == "deflate":
        comp = COMP_DEFLATE
    else:
        raise ValueError(f"compress = {compress!r}: None, 'none' and 'deflate' are written")
    if bits not in (8, 16):
        raise ValueError(f"{bits}-bit samples: only unsigned 8- and 16-bit samples are written tiled or compressed")
    if planar not in (1, 2):
        raise ValueError(f"planar = {planar}: 1 (chunky) or 2 (planar)")
    if predictor is None:
        predictor = 2 if comp == COMP_DEFLATE else 1
    if predictor not in (1, 2):
        raise ValueError(f"predictor = {predictor}: 1 (none) or 2 (horizontal differencing)")
    if comp == COMP_NONE and predictor != 1:
        raise ValueError("predictor 2 goes with Deflate: readers ignore the tag on uncompressed data")
    if tile is not None and rows_per_strip is not None:
        raise ValueError("tile and rows_per_strip exclude each other")
    if rows_per_strip is not None:
        if not 1 <= int(rows_per_strip):
            raise ValueError(f"rows_per_strip = {rows_per_strip}: at least 1")
        tiled, sw, sh = 0, W, min(int(rows_per_strip), H)
    else:
        tw, th = (tile, tile) if np.isscalar(tile) else (DEFAULT_TILE, DEFAULT_TILE) if tile is None else tile
        for side in (tw, th):
            if int(side) != side or side < 16 or side % 16:
                raise ValueError(f"tile side {side}: TIFF 6.0 wants a positive multiple of 16")
        tiled, sw, sh = 1, int(tw), int(th)
    lay = Layout(C, H, W, bits, 0, planar, sw, sh, tiled, comp, predictor)
    if cap is None:
        cap = lib().lbdrn_tiffw_segment_cap(comp)
    if segment_bytes(lay) > cap:
        raise ValueError(f"a segment of {segment_bytes(lay)} bytes ({sw} x {sh}) is above the cap of {cap} bytes for "
                         f"compress = {compress!r}: use smaller tiles or fewer rows per strip")
    return lay


# ---------------------------------------------------------------- the container

BIG_LIMIT = 0xFFFFFFFF


def assemble(lay, counts, sample_format=1, force_big=False, body_bytes=None):
    """The bytes in front of the first segment -- header, IFD, out-of-line values, the segment tables -- and the file offset
    of every segment, the segments following back to back.  BigTIFF when force_big or when the end of the last segment
    (body_bytes, default sum(counts)) would pass 2^32 - 1."""
    counts = [int(c) for c in counts]
    body = sum(counts) if body_bytes is None else int(body_bytes)
    C, n = lay.C, len(counts)
    for big in ((True,) if force_big else (False, True)):
        lt = 16 if big else 4      # LONG8 / LONG for offsets and counts
        # three or more 8-bit bands are RGB (and extra samples), as GDAL's GTiff driver has it: libtiff-based viewers know no
        # other way to show them; everything else is min-is-black with C - 1 extra samples, as _write_tiff writes it
        rgb = lay.bits == 8 and C >= 3
        entries = [(256, 4, [lay.W]), (257, 4, [lay.H]), (258, 3, [lay.bits] * C), (259, 3, [lay.compression]), (262, 3, [2 if rgb else 1])]
        if not lay.tiled:
            entries += [(273, lt, None), (277, 3, [C]), (278, 4, [lay.seg_h]), (279, lt, counts)]
        else:
            entries += [(277, 3, [C])]
        entries.append((284, 3, [lay.planar]))
        if lay.predictor == 2:
            entries.append((317, 3, [2]))
        if lay.tiled:
            entries += [(322, 4, [lay.seg_w]), (323, 4, [lay.seg_h]), (324, lt, None), (325, lt, counts)]
        if C > (3 if rgb else 1):
            entries.append((338, 3, [0] * (C - (3 if rgb else 1))))
        entries.append((339, 3, [sample_format] * C))
        entries.sort(key=lambda e: e[0])
        if big:
            head, ent, inline = 16, 20, 8
            ifd_size = 8 + ent * len(entries) + 8
        else:
            head, ent, inline = 8, 12, 4
            ifd_size = 2 + ent * len(entries) + 4
        size = {3: 2, 4: 4, 16: 8}
        code = {3: "H", 4: "I", 16: "Q"}
        at = head + ifd_size      # out-of-line values follow the IFD
        where = {}
        for tag, typ, vals in entries:
            nbytes = size[typ] * (n if vals is None else len(vals))
            if nbytes > inline:
                where[tag] = at
                at += nbytes + (nbytes & 1)
        data_off = at + (at & 1)
        if not big and data_off + body > BIG_LIMIT:
            continue
        offsets, o = [], data_off
        for c in counts:
            offsets.append(o)
            o += c
        out = bytearray(data_off)
        if big:
            struct.pack_into("<2sHHHQ", out, 0, b"II", 43, 8, 0, head)
            struct.pack_into("<Q", out, head, len(entries))
            p = head + 8
        else:
            struct.pack_into("<2sHI", out, 0, b"II", 42, head)
            struct.pack_into("<H", out, head, len(entries))
            p = head + 2
        for tag, typ, vals in entries:
            vals = offsets if vals is None else vals
            raw = struct.pack("<%d%s" % (len(vals), code[typ]), *vals)
            struct.pack_into("<HH" + ("Q" if big else "I"), out, p, tag, typ, len(vals))
            vp = p + (12 if big else 8)
            if tag in where:
                struct.pack_into("<" + ("Q" if big else "I"), out, vp, where[tag])
                out[where[tag]:where[tag] + len(raw)] = raw
            else:
                out[vp:vp + len(raw)] = raw
            p += ent
        return bytes(out), offsets
    raise AssertionError("unreachable")


# ---------------------------------------------------------------- the container of a pyramidal or georeferenced file

_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8}


def _level_entries(lay, counts, lt, sample_format, overview, geo):
    """the entries of one IFD as (tag, type, count, value bytes or None for the segment offsets), in ascending tag order: the
    tags assemble() writes for `lay`, NewSubfileType = 1 on an overview, the `geo` tags on the full-resolution IFD"""
    C = lay.C
    code = {3: "H", 4: "I", 16: "Q"}
    rgb = lay.bits == 8 and C >= 3
    entries = [(256, 4, [lay.W]), (257, 4, [lay.H]), (258, 3, [lay.bits] * C), (259, 3, [lay.compression]), (262, 3, [2 if rgb else 1])]
    if overview:
        entries.append((254, 4, [1]))
    if not lay.tiled:
        entries += [(273, lt, None), (277, 3, [C]), (278, 4, [lay.seg_h]), (279, lt, counts)]
    else:
        entries += [(277, 3, [C])]
    entries.append((284, 3, [lay.planar]))
    if lay.predictor == 2:
        entries.append((317, 3, [2]))
    if lay.tiled:
        entries += [(322, 4, [lay.seg_w]), (323, 4, [lay.seg_h]), (324, lt, None), (325, lt, counts)]
    if C > (3 if rgb else 1):
        entries.append((338, 3, [0] * (C - (3 if rgb else 1))))
    entries.append((339, 3, [sample_format] * C))
    out = [(tag, typ, len(counts) if vals is None else len(vals), None if vals is None else struct.pack("<%d%s" % (len(vals), code[typ]), *vals))
           for tag, typ, vals in entries]
    taken = {e[0] for e in out} | {254, 273, 278, 279, 317, 322, 323, 324, 325, 338}
    for item in (geo or ()):
        try:
            tag, typ, cnt, raw = item
            tag, typ, cnt, raw = int(tag), int(typ), int(cnt), bytes(raw)
        except (TypeError, ValueError):
            raise ValueError(f"geo: {item!r} is no (tag, type, count, value bytes)") from None
        if not 0 < tag < 65536 or tag in taken:
            raise ValueError(f"geo: tag {tag} is one the writer sets itself, is given twice or is no tag")
        if typ not in _TYPE_SIZE or cnt < 1 or len(raw) != _TYPE_SIZE[typ] * cnt:
            raise ValueError(f"geo: tag {tag}: {len(raw)} value bytes for {cnt} values of type {typ}")
        taken.add(tag)
        out.append((tag, typ, cnt, raw))
    out.sort(key=lambda e: e[0])
    return out


def assemble_pyramid(lays, counts_per_level, geo=None, sample_format=1, force_big=False, body_bytes=None):
    """The container of a file of several levels: lays[0] / counts_per_level[0] the full resolution, then the overviews in
    decreasing size.  Returns (head bytes, [segment offsets of every level]).  The head holds the header, then every IFD
    followed by its out-of-line values and segment tables, chained in the order given; overview IFDs carry NewSubfileType = 1
    and `geo` -- [(tag, type, count, little-endian value bytes)] -- goes on the first IFD alone.  The segments follow the
    head, those of the LAST (smallest) level first and the full resolution last, each level's back to back.  BigTIFF when
    force_big or when the end of the last segment would pass 2^32 - 1; body_bytes: the bytes of every level's segments
    (default: the sums of its counts).  One level and no geo: exactly assemble()."""
    lays = list(lays)
    counts_per_level = [[int(c) for c in counts] for counts in counts_per_level]
    if len(lays) != len(counts_per_level) or not lays:
        raise ValueError("assemble_pyramid: one list of counts for every layout, and at least one layout")
    bodies = [sum(c) for c in counts_per_level] if body_bytes is None else [int(b) for b in body_bytes]
    if len(bodies) != len(lays):
        raise ValueError("assemble_pyramid: one body size for every layout")
    if len(lays) == 1 and not geo:
        head, offsets = assemble(lays[0], counts_per_level[0], sample_format, force_big, bodies[0])
        return head, [offsets]
    for big in ((True,) if force_big else (False, True)):
        lt = 16 if big else 4
        head, ent, inline, cnt_size, nxt_size = (16, 20, 8, 8, 8) if big else (8, 12, 4, 2, 4)
        levels = []      # (IFD offset, entries, {tag: offset of its out-of-line value})
        at = head
        for k, (lay, counts) in enumerate(zip(lays, counts_per_level)):
            entries = _level_entries(lay, counts, lt, sample_format, k > 0, geo if k == 0 else None)
            ifd_at = at
            at += cnt_size + ent * len(entries) + nxt_size
            where = {}
            for tag, typ, cnt, raw in entries:
                nbytes = _TYPE_SIZE[typ] * cnt
                if nbytes > inline:
                    where[tag] = at
                    at += nbytes + (nbytes & 1)
            levels.append((ifd_at, entries, where))
        data_off = at + (at & 1)
        if not big and data_off + sum(bodies) > BIG_LIMIT:
            continue
        starts, o = [0] * len(lays), data_off
        for k in reversed(range(len(lays))):      # smallest level first
            starts[k] = o
            o += bodies[k]
        all_offsets = []
        for k, counts in enumerate(counts_per_level):
            offsets, o = [], starts[k]
            for c in counts:
                offsets.append(o)
                o += c
            all_offsets.append(offsets)
        out = bytearray(data_off)
        word = "Q" if big else "I"
        if big:
            struct.pack_into("<2sHHHQ", out, 0, b"II", 43, 8, 0, head)
        else:
            struct.pack_into("<2sHI", out, 0, b"II", 42, head)
        for k, (ifd_at, entries, where) in enumerate(levels):
            struct.pack_into("<" + ("Q" if big else "H"), out, ifd_at, len(entries))
            p = ifd_at + cnt_size
            for tag, typ, cnt, raw in entries:
                if raw is None:
                    raw = struct.pack("<%d%s" % (cnt, word), *all_offsets[k])
                struct.pack_into("<HH" + word, out, p, tag, typ, cnt)
                vp = p + (12 if big else 8)
                if tag in where:
                    struct.pack_into("<" + word, out, vp, where[tag])
                    out[where[tag]:where[tag] + len(raw)] = raw
                else:
                    out[vp:vp + len(raw)] = raw
                p += ent
            struct.pack_into("<" + word, out, p, levels[k + 1][0] if k + 1 < len(levels) else 0)
        return bytes(out), all_offsets
    raise AssertionError("unreachable")


# ---------------------------------------------------------------- the device stage

def encode_device(tensor, lay):
    """The segments of `tensor` ([C,H,W] in HBM) under `lay`: (body, offsets, counts) -- the segments' bytes back to back as
    a numpy uint8 array, and where each lies in it.  Only the table and body[:total] are downloaded."""
    import torch
    L = lib()
    nseg = L.lbdrn_tiffw_segment_count(ctypes.byref(lay))
    if not nseg:
        raise TiffWriteError("the layout is out of the library's range")
    want = torch.uint8 if lay.bits == 8 else torch.int16
    if tensor.dtype != want or tuple(tensor.shape) != (lay.C, lay.H, lay.W) or not tensor.is_cuda:
        raise TiffWriteError(f"planes: a {want} tensor of shape {(lay.C, lay.H, lay.W)} in device memory is expected")
    planes = tensor.contiguous()
    dev = planes.device
    nout = L.lbdrn_tiffw_output_bytes(ctypes.byref(lay))
    nws = L.lbdrn_tiffw_workspace(ctypes.byref(lay))
    with torch.cuda.device(dev):
        out = torch.empty(max(nout, 1), dtype=torch.uint8, device=dev)
        table = torch.empty(2 * nseg + 1, dtype=torch.int64, device=dev)      # offsets, counts, total
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
        base = table.data_ptr()
        _check(L.lbdrn_tiffw_encode(ctypes.byref(lay), planes.data_ptr(), out.data_ptr(), nout, base, base + 8 * nseg,
                                    base + 16 * nseg, ws.data_ptr(), nws, torch.cuda.current_stream(dev).cuda_stream),
               "lbdrn_tiffw_encode")
        tab = table.cpu().numpy().view(np.uint64)      # the one host sync
        total = int(tab[2 * nseg])
        body = out[:total].cpu().numpy()
    return body, tab[:nseg].copy(), tab[nseg:2 * nseg].copy()


def _encode_levels(planes, lays):
    """encode_device of every level, side by side: the full resolution on the caller's stream and each overview on a stream of
    its own, each from a host thread of its own (encode_device ends in a download).  A level of few segments costs the time
    of one wave on one segment whatever its size, and the levels do not depend on each other; the streams wait for the
    caller's, on which the levels were reduced."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    if len(planes) == 1:
        return [encode_device(planes[0], lays[0])]
    dev = planes[0].device
    main = torch.cuda.current_stream(dev)
    streams = [main] + [torch.cuda.Stream(device=dev) for _ in planes[1:]]
    for s in streams[1:]:
        s.wait_stream(main)

    def one(k):
        with torch.cuda.device(dev), torch.cuda.stream(streams[k]):      # (the current stream is a thread's own)
            return encode_device(planes[k], lays[k])
    with ThreadPoolExecutor(len(planes)) as pool:
        return list(pool.map(one, range(len(planes))))


def write_segments(path, lay, body, counts, sample_format=1):
    head, _ = assemble(lay, counts, sample_format)
    with open(path, "wb") as f:
        f.write(head)
        f.write(memoryview(np.ascontiguousarray(body)))


def check_pyramid_options(H, W, bits, tile, rows_per_strip, overviews, resampling, nodata, geo):
    """The refusals of the overview and georeferencing options, before any device work: the sizes [(H_k, W_k)] of the levels
    to write (none where overviews is None or 0)."""
    from . import pyramid
    pyramid.check_options(resampling, nodata, bits)
    if overviews is None:
        if nodata is not None:
            raise ValueError("nodata enters the overviews' averages only: give overviews with it")
        return []
    if rows_per_strip is not None:
        raise ValueError("overviews go with tiles: rows_per_strip and overviews exclude each other")
    return pyramid.level_sizes(H, W, overviews, tile)


def write_device(path, tensor, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None, overviews=None,
                 resampling="average", nodata=None, geo=None):
    """`tensor`: [C,H,W] in HBM, int16 storage for 16-bit samples, uint8 for 8-bit ones.  overviews: "auto" or a count --
    the levels are reduced on the device (lbdrn_hip.pyramid: resampling, nodata) from the planes where they lie, each coded
    like the full resolution, and the file holds one IFD per level; geo: [(tag, type, count, little-endian value bytes)], as
    tiff.read_geo_tags returns them, written on the full-resolution IFD.  With neither, the file is what it always was."""
    import torch
    if tensor.dim() != 3 or tensor.dtype not in (torch.uint8, torch.int16):
        raise ValueError("write_device takes a [C,H,W] tensor of uint8, or of int16 holding unsigned 16-bit samples")
    C, H, W = (int(v) for v in tensor.shape)
    bits = 8 if tensor.dtype == torch.uint8 else 16
    lay = make_layout(C, H, W, bits, compress, tile, rows_per_strip, planar, predictor)
    sizes = check_pyramid_options(H, W, bits, tile, rows_per_strip, overviews, resampling, nodata, geo)
    if not sizes and not geo:
        body, _, counts = encode_device(tensor, lay)
        write_segments(path, lay, body, counts)
        return lay
    lays = [lay] + [make_layout(C, h, w, bits, compress, tile, None, planar, predictor) for h, w in sizes]
    assemble_pyramid(lays, [[0] * segment_count(l) for l in lays], geo)      # (the refusals of `geo` come before the device work)
    planes = [tensor]
    if sizes:
        from . import pyramid
        planes += pyramid.build(tensor, len(sizes), resampling, nodata)
    coded = _encode_levels(planes, lays)
    bodies, counts = [c[0] for c in coded], [c[2] for c in coded]
    head, _ = assemble_pyramid(lays, counts, geo)
    with open(path, "wb") as f:
        f.write(head)
        for body in reversed(bodies):      # smallest level first, the full resolution last
            f.write(memoryview(np.ascontiguousarray(body)))
    return lay


def write(path, array, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None, device=None, overviews=None,
          resampling="average", nodata=None, geo=None):
    """numpy uint8 / uint16 [C,H,W] (or [H,W]): uploaded once, then write_device."""
    import torch
    a = np.ascontiguousarray(array if array.ndim == 3 else array[None])
    if a.dtype.type not in (np.uint8, np.uint16):
        raise ValueError(f"{a.dtype} samples: only uint8 and uint16 rasters are written tiled or compressed")
    # the layout's own refusals come before the device is asked for
    make_layout(a.shape[0], a.shape[1], a.shape[2], a.dtype.itemsize * 8, compress, tile, rows_per_strip, planar, predictor)
    check_pyramid_options(a.shape[1], a.shape[2], a.dtype.itemsize * 8, tile, rows_per_strip, overviews, resampling, nodata, geo)
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise TiffWriteError("a tiled or compressed TIFF is built on the GPU; there is no CPU path in this package")
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    return write_device(path, t, compress, tile, rows_per_strip, planar, predictor, overviews, resampling, nodata, geo)
