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
Georeferencing tags and overviews are not written."""
import ctypes
import os
import struct

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PATH = os.environ.get("LBDRN_TIFFW_LIB") or os.path.join(os.path.dirname(_HERE), "liblbdrn_tiffw.so")
ABI_VERSION = 1
E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4      # lbdrn_status of include/lbdrn_hip.h
COMP_NONE, COMP_DEFLATE = 1, 8
DEFAULT_TILE = 256

_lib = None


class TiffWriteError(RuntimeError):
    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class Layout(ctypes.Structure):
    """lbdrn_tiffw_layout"""
    _fields_ = [(n, ctypes.c_int32) for n in ("C", "H", "W", "bits", "big_endian", "planar", "seg_w", "seg_h", "tiled",
                                              "compression", "predictor")]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise TiffWriteError(f"{_PATH} not built (python lbdrn-msic_amd/csrc/build.py)")
        L = ctypes.CDLL(_PATH)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        lp = ctypes.POINTER(Layout)
        L.lbdrn_tiffw_last_error.restype = ctypes.c_char_p
        L.lbdrn_tiffw_abi_version.restype = ctypes.c_int
        for name, args in (("segment_count", [lp]), ("segment_cap", [ctypes.c_int32]), ("bound", [sz]), ("block_tokens", []),
                           ("output_bytes", [lp]), ("workspace", [lp])):
            f = getattr(L, "lbdrn_tiffw_" + name)
            f.argtypes, f.restype = args, sz
        L.lbdrn_tiffw_encode.argtypes = [lp, vp, vp, sz, vp, vp, vp, vp, sz, vp]
        if L.lbdrn_tiffw_abi_version() != ABI_VERSION:
            raise TiffWriteError(f"{_PATH}: ABI version {L.lbdrn_tiffw_abi_version()}, this binding is for {ABI_VERSION}")
        _lib = L
    return _lib


def available():
    try:
        lib()
        return True
    except (TiffWriteError, OSError):
        return False


def _check(rc, what):
    if rc != 0:
        raise TiffWriteError(f"{what}: {(lib().lbdrn_tiffw_last_error() or b'').decode(errors='replace')}", rc)


# ---------------------------------------------------------------- the layout of a call

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


def write_segments(path, lay, body, counts, sample_format=1):
    head, _ = assemble(lay, counts, sample_format)
    with open(path, "wb") as f:
        f.write(head)
        f.write(memoryview(np.ascontiguousarray(body)))


def write_device(path, tensor, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None):
    """`tensor`: [C,H,W] in HBM, int16 storage for 16-bit samples, uint8 for 8-bit ones."""
    import torch
    if tensor.dim() != 3 or tensor.dtype not in (torch.uint8, torch.int16):
        raise ValueError("write_device takes a [C,H,W] tensor of uint8, or of int16 holding unsigned 16-bit samples")
    C, H, W = (int(v) for v in tensor.shape)
    lay = make_layout(C, H, W, 8 if tensor.dtype == torch.uint8 else 16, compress, tile, rows_per_strip, planar, predictor)
    body, _, counts = encode_device(tensor, lay)
    write_segments(path, lay, body, counts)
    return lay


def write(path, array, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None, device=None):
    """numpy uint8 / uint16 [C,H,W] (or [H,W]): uploaded once, then write_device."""
    import torch
    a = np.ascontiguousarray(array if array.ndim == 3 else array[None])
    if a.dtype.type not in (np.uint8, np.uint16):
        raise ValueError(f"{a.dtype} samples: only uint8 and uint16 rasters are written tiled or compressed")
    # the layout's own refusals come before the device is asked for
    make_layout(a.shape[0], a.shape[1], a.shape[2], a.dtype.itemsize * 8, compress, tile, rows_per_strip, planar, predictor)
    dev = torch.device(device if device is not None else "cuda:0")
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise TiffWriteError("a tiled or compressed TIFF is built on the GPU; there is no CPU path in this package")
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    return write_device(path, t, compress, tile, rows_per_strip, planar, predictor)
