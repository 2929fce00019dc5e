"""Raster files in and out (the reference goes through GDAL: LBDRNdataset.py:71-89, 93).

GDAL is used when it is importable.  Without it this module reads and writes the subset the codec
itself produces and consumes: baseline TIFF, uncompressed strips, unsigned 8/16-bit or float32
samples, any band count, chunky or planar, either byte order -- and .npy arrays.  Every other TIFF
-- BigTIFF, tiles, LZW / Deflate / PackBits, predictor 2 -- goes to lbdrn_hip.tiff, which parses it on
the host and decompresses its segments on the GPU.  Arrays are [C,H,W] (or [H,W] for one band), as
gdal's ReadAsArray() returns them.  write_raster with a compression or tiling option, and write_raster_device,
go to lbdrn_hip.tiff_write, which builds and Deflate-compresses the segments on the GPU -- with overviews= the overview
levels too, reduced on the GPU by lbdrn_hip.pyramid, and with geo= the georeferencing tags read_geo_tags copied from
another file.  read_raster(path, overview=k) reads level k of such a file.
read_raster(path, window=(x0, y0, w, h)) and read_raster_device(..., window=) read that part alone, equal to the same slice of the
whole read, from a read-only memory map: only the strips or tiles the window touches are read, uploaded and decoded
(lbdrn_hip.tiff.plan_window); raster_shape(path) tells (C, H, W, dtype) from the tags.
"""
import struct

import numpy as np

_TYPES = {1: "B", 2: "c", 3: "H", 4: "I", 5: "II", 16: "Q"}


def _gdal():
    try:
        from osgeo import gdal
        gdal.UseExceptions()
        return gdal
    except Exception:
        return None


def _overview_ifd(buf, path, overview):
    """the chain position of overview level `overview` >= 1: the IFDs whose NewSubfileType has bit 0 set, in file order"""
    from . import tiff
    levels = tiff.overview_ifds(buf, path)
    if not 1 <= overview <= len(levels):
        raise IndexError(f"{path}: overview {overview} of a file that has {len(levels)} overview level{'s' * (len(levels) != 1)}")
    return levels[overview - 1]


def _check_overview(path, overview):
    if isinstance(overview, bool) or int(overview) != overview or overview < 0:
        raise ValueError(f"overview = {overview!r}: 0 (the full resolution) or the number of a level")
    if overview and path.endswith(".npy"):
        raise IndexError(f"{path}: overview {overview} of a .npy array, which has no overview levels")
    return int(overview)


def read_raster(path, overview=0, window=None):
    """overview=k >= 1: level k of a pyramidal TIFF, through this package's parser and the GPU reader even where GDAL
    imports; IndexError where the file has fewer levels.  window=(x0, y0, w, h): that part of the raster (of level k) alone,
    equal to the same slice of the whole read, without reading or decoding the rest of the file (_read_window)."""
    if window is not None:
        return _read_window(path, _check_overview(path, overview), window, None)
    if _check_overview(path, overview):
        from . import tiff
        with open(path, "rb") as f:
            buf = f.read()
        return tiff.read(path, ifd=_overview_ifd(buf, path, overview))
    if path.endswith(".npy"):
        return np.load(path)
    g = _gdal()
    if g is not None:
        return g.Open(path).ReadAsArray()
    return _read_tiff(path)


def read_raster_device(path, device="cuda:0", overview=0, window=None):
    """The raster as a contiguous [C,H,W] tensor on `device`, for callers that want the planes left in HBM: 16-bit samples as
    int16 storage, like every plane of this package.  A tiled or compressed TIFF never passes through host arrays.
    overview=k >= 1: level k of a pyramidal TIFF, as read_raster has it; window=(x0, y0, w, h): that part alone, [C,h,w]."""
    import torch
    if window is not None:
        return _read_window(path, _check_overview(path, overview), window, device)
    if _check_overview(path, overview):
        from . import tiff
        with open(path, "rb") as f:
            buf = f.read()
        return tiff.read_device_bytes(buf, path, device, ifd=_overview_ifd(buf, path, overview))
    a = None
    if path.endswith(".npy") or _gdal() is not None:
        a = read_raster(path)
    else:
        from . import tiff
        with open(path, "rb") as f:
            buf = f.read()
        try:
            scene = tiff.parse(buf, path)
        except ValueError:
            scene = None      # float samples and the like: this module's own reader takes them or says why not
        if scene is None or (scene.plain_strips() and buf[2:4] in (b"*\0", b"\0*")):
            a = _read_tiff(path)
        else:
            return tiff.read_device_bytes(buf, path, device)
    a = np.ascontiguousarray(a if a.ndim == 3 else a[None])
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _classic_plain(buf):
    """(tags, byte order, dtype, C, H, W, planar) of a file _read_tiff reads by itself -- a classic TIFF of uncompressed
    strips -- or None.  Reads the header, the IFD and the tag arrays through slices: buf may be a memory map."""
    bo = {b"II": "<", b"MM": ">"}.get(bytes(buf[:2]))
    if bo is None or len(buf) < 8 or struct.unpack(bo + "H", buf[2:4])[0] != 42:
        return None
    off = struct.unpack(bo + "I", buf[4:8])[0]
    n = struct.unpack(bo + "H", buf[off:off + 2])[0]
    tags = {}
    for i in range(n):
        tag, typ, cnt, val = struct.unpack(bo + "HHI4s", buf[off + 2 + 12 * i:off + 14 + 12 * i])
        size = {1: 1, 3: 2, 4: 4}.get(typ)
        if size is None:
            continue
        at = struct.unpack(bo + "I", val)[0]
        raw = val if size * cnt <= 4 else buf[at:at + size * cnt]
        tags[tag] = list(struct.unpack(bo + f"{cnt}" + {1: "B", 3: "H", 4: "I"}[typ], raw[:size * cnt]))
    if tags.get(259, [1])[0] != 1 or 322 in tags:
        return None
    bits = tags.get(258, [1])
    if len(set(bits)) != 1:
        raise ValueError("mixed bit depths")
    dt = {(8, 1): "u1", (16, 1): "u2", (32, 1): "u4", (32, 3): "f4", (64, 3): "f8"}[(bits[0], tags.get(339, [1])[0])]
    return tags, bo, np.dtype(bo + dt), tags.get(277, [1])[0], tags[257][0], tags[256][0], tags.get(284, [1])[0]


def _window_of_strips(buf, plain, window):
    """_read_tiff's array, windowed: _read_tiff joins the strips and reshapes, so row y of band b lies at a known place of
    the joined stream; only the window's rows are taken from the file, then the columns are sliced"""
    tags, bo, dt, C, H, W, planar = plain
    x0, y0, w, h = window
    offs, cnts = tags[273], tags[279]
    starts = np.concatenate([[0], np.cumsum(cnts)])

    def joined(a, b):      # bytes [a, b) of the strips one after another
        out, k = [], int(np.searchsorted(starts, a, side="right")) - 1
        while a < b and k < len(offs):
            n = min(b, int(starts[k + 1])) - a
            out.append(buf[offs[k] + a - int(starts[k]):offs[k] + a - int(starts[k]) + n])
            a, k = a + n, k + 1
        return b"".join(out)
    if planar == 2:
        row = W * dt.itemsize
        a = np.stack([np.frombuffer(joined((b * H + y0) * row, (b * H + y0 + h) * row), dt).reshape(h, W) for b in range(C)])
    else:
        row = W * C * dt.itemsize
        a = np.frombuffer(joined(y0 * row, (y0 + h) * row), dt).reshape(h, W, C).transpose(2, 0, 1)
    a = np.ascontiguousarray(a[:, :, x0:x0 + w].astype(dt.newbyteorder("=")))
    return a[0] if C == 1 else a


def raster_shape(path, overview=0):
    """(C, H, W, dtype) of what read_raster(path, overview) returns, C = 1 for an [H,W] result; no pixel data is read"""
    overview = _check_overview(path, overview)
    if path.endswith(".npy"):
        a = np.load(path, mmap_mode="r")
        return ((1,) if a.ndim == 2 else ()) + tuple(a.shape) + (a.dtype,)
    g = _gdal()
    if g is not None and not overview:
        from osgeo import gdal_array
        ds = g.Open(path)
        return (ds.RasterCount, ds.RasterYSize, ds.RasterXSize,
                np.dtype(gdal_array.GDALTypeCodeToNumericTypeCode(ds.GetRasterBand(1).DataType)))
    from . import tiff
    buf = tiff.open_map(path)
    try:
        plain = None if overview else _classic_plain(buf)
        if plain is not None:
            return plain[3], plain[4], plain[5], plain[2].newbyteorder("=")
        lay = tiff._parse(buf, path, _overview_ifd(buf, path, overview) if overview else 0, False).layout
        return lay.C, lay.H, lay.W, np.dtype(np.uint8 if lay.bits == 8 else np.uint16)
    finally:
        if not isinstance(buf, bytes):
            buf.close()


def _read_window(path, overview, window, device):
    """read_raster (device None) and read_raster_device with a window: the same slice of the whole read, same dtype, [h,w]
    for one band where read_raster returns [H,W].  A .npy array is memory-mapped; GDAL reads the window where it imports and
    the full resolution is asked for; everything else is read from a read-only memory map of the file, this module's own
    uncompressed strips by their rows, the rest through tiff.read_window_bytes -- only the touched segments are uploaded."""
    from .codec import check_window
    a = None
    if path.endswith(".npy"):
        m = np.load(path, mmap_mode="r")
        x0, y0, w, h = check_window(window, m.shape[-1], m.shape[-2])
        a = np.array(m[..., y0:y0 + h, x0:x0 + w])
    elif _gdal() is not None and not overview:
        ds = _gdal().Open(path)
        a = ds.ReadAsArray(*check_window(window, ds.RasterXSize, ds.RasterYSize))
    else:
        from . import tiff
        buf = tiff.open_map(path)
        try:
            plain = None if overview else _classic_plain(buf)
            if plain is not None:
                a = _window_of_strips(buf, plain, check_window(window, plain[5], plain[4]))
            elif device is not None:
                return tiff.read_window_bytes(buf, path, window, device, _overview_ifd(buf, path, overview) if overview else 0)
            else:
                a = tiff._window(buf, path, window, None, _overview_ifd(buf, path, overview) if overview else 0, False)
                a = a[0] if a.shape[0] == 1 else a
        finally:
            if not isinstance(buf, bytes):
                buf.close()
    if device is None:
        return a
    import torch
    a = np.ascontiguousarray(a if a.ndim == 3 else a[None])
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def read_geo_tags(path):
    """The georeferencing tags of a TIFF's first IFD as [(tag, type, count, little-endian value bytes)] -- what write_raster
    takes as `geo`; [] for a file without them and for a .npy array.  Read from a read-only memory map: only the header,
    the IFD and the tags' values are touched, whatever the size of the scene."""
    if path.endswith(".npy"):
        return []
    from . import tiff
    buf = tiff.open_map(path)
    try:
        return tiff.read_geo_tags(buf, path)
    finally:
        if not isinstance(buf, bytes):
            buf.close()


def _wants_writer(path, compress, tile, rows_per_strip, planar, predictor, overviews=None, resampling="average", nodata=None, geo=None):
    """whether the options of a write ask for lbdrn_hip.tiff_write (anything but today's uncompressed planar strips)"""
    new = overviews is not None or resampling != "average" or nodata is not None or geo is not None
    if compress is None and tile is None and rows_per_strip is None and planar == 2 and predictor is None and not new:
        return False
    if path.endswith(".npy"):
        if new:
            raise ValueError("overviews, resampling, nodata and geo are options of a TIFF, not of a .npy array")
        raise ValueError("compress, tile, rows_per_strip, planar and predictor are options of a TIFF, not of a .npy array")
    if compress not in (None, "none", "deflate"):
        raise ValueError(f"compress = {compress!r}: None, 'none' and 'deflate' are written")
    return True


def _new_options(overviews, resampling, nodata, geo):
    """the overview and georeferencing options that were given, as keywords: a write without them is the call it always was"""
    given = {"overviews": overviews, "nodata": nodata, "geo": geo}
    out = {k: v for k, v in given.items() if v is not None}
    if resampling != "average":
        out["resampling"] = resampling
    return out


def write_raster(path, array, compress=None, tile=None, rows_per_strip=None, planar=2, predictor=None, overviews=None,
                 resampling="average", nodata=None, geo=None, device=None):
    """array [C,H,W]: uint8 / uint16 / float32 / float64 (ref write_tiff_with_gdal).  With every option at its default the
    file is what it always was: one uncompressed strip per band.  compress="deflate" (defaults: 256 x 256 tiles, planar,
    predictor 2), or compress=None with tile= or rows_per_strip=, writes through lbdrn_hip.tiff_write: the array is uploaded
    and its segments are built and compressed on the GPU.  Integer rasters only.  overviews="auto" or a count adds that many
    overview levels, reduced on the GPU (resampling "average" or "nearest", nodata a value that does not enter an average);
    geo -- what read_geo_tags returns -- is copied onto the full-resolution IFD.  Either goes through the same writer, on
    `device` (default "cuda:0")."""
    if array.dtype.type not in (np.uint8, np.uint16, np.float32, np.float64):
        raise ValueError("Unsupported data type in this function")
    if _wants_writer(path, compress, tile, rows_per_strip, planar, predictor, overviews, resampling, nodata, geo):
        if array.dtype.kind == "f":
            raise ValueError(f"{array.dtype} rasters are written uncompressed only: compress, tile, rows_per_strip, planar and "
                             "predictor are for uint8 / uint16 (the reader reads no compressed float raster either)")
        from . import tiff_write
        tiff_write.write(path, array, compress or "none", tile, rows_per_strip, planar, predictor, device,
                         **_new_options(overviews, resampling, nodata, geo))
        return
    if path.endswith(".npy"):
        np.save(path, array)
        return
    g = _gdal()
    if g is not None:
        code = {np.uint8: g.GDT_Byte, np.uint16: g.GDT_UInt16, np.float32: g.GDT_Float32,
                np.float64: g.GDT_Float64}[array.dtype.type]
        ds = g.GetDriverByName("GTiff").Create(path, array.shape[2], array.shape[1], array.shape[0], code)
        for i in range(array.shape[0]):
            ds.GetRasterBand(i + 1).WriteArray(array[i])
        ds.FlushCache()
        return
    _write_tiff(path, array)


def write_raster_device(path, tensor, compress="deflate", tile=None, rows_per_strip=None, planar=2, predictor=None, overviews=None,
                        resampling="average", nodata=None, geo=None):
    """write_raster for a [C,H,W] tensor that sits in HBM (int16 storage for 16-bit samples, uint8 for 8-bit ones): the
    segments are built and compressed where the planes lie, and only the compressed bytes are downloaded.  A .npy path
    takes the host copy it cannot avoid."""
    if path.endswith(".npy"):
        _wants_writer(path, None if compress in (None, "none") else compress, tile, rows_per_strip, planar, predictor, overviews,
                      resampling, nodata, geo)
        a = tensor.cpu().numpy()
        np.save(path, a.view(np.uint16) if a.dtype == np.int16 else a)
        return
    _wants_writer(path, compress, tile, rows_per_strip, planar, predictor, overviews, resampling, nodata, geo)
    from . import tiff_write
    tiff_write.write_device(path, tensor, compress or "none", tile, rows_per_strip, planar, predictor,
                            **_new_options(overviews, resampling, nodata, geo))


def raster_size(path):
    a = read_raster(path)
    return a.shape[-1], a.shape[-2]


def _read_tiff_device(path):
    """what _read_tiff does not read by itself: parsed on the host, decompressed on the GPU (lbdrn_hip/tiff.py)"""
    from . import tiff
    return tiff.read(path)


def _read_tiff(path):
    with open(path, "rb") as f:
        buf = f.read()
    bo = {b"II": "<", b"MM": ">"}.get(buf[:2])
    if bo is None or struct.unpack_from(bo + "H", buf, 2)[0] != 42:
        return _read_tiff_device(path)      # BigTIFF; anything that is no TIFF at all raises there
    off = struct.unpack_from(bo + "I", buf, 4)[0]
    n = struct.unpack_from(bo + "H", buf, off)[0]
    tags = {}
    for i in range(n):
        tag, typ, cnt, val = struct.unpack_from(bo + "HHI4s", buf, off + 2 + 12 * i)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 16: 8}.get(typ)
        if size is None:
            continue
        raw = val if size * cnt <= 4 else buf[struct.unpack(bo + "I", val)[0]:][:size * cnt]
        if typ == 3:
            tags[tag] = list(struct.unpack(bo + f"{cnt}H", raw[:2 * cnt]))
        elif typ == 4:
            tags[tag] = list(struct.unpack(bo + f"{cnt}I", raw[:4 * cnt]))
        elif typ == 1:
            tags[tag] = list(raw[:cnt])
    W, H = tags[256][0], tags[257][0]
    bits = tags.get(258, [1])
    spp = tags.get(277, [1])[0]
    if tags.get(259, [1])[0] != 1:
        return _read_tiff_device(path)
    if 322 in tags:
        return _read_tiff_device(path)
    fmt = tags.get(339, [1])[0]
    planar = tags.get(284, [1])[0]
    if len(set(bits)) != 1:
        raise ValueError("mixed bit depths")
    dt = {(8, 1): "u1", (16, 1): "u2", (32, 1): "u4", (32, 3): "f4", (64, 3): "f8"}[(bits[0], fmt)]
    dt = np.dtype(bo + dt)
    data = b"".join(buf[o:o + c] for o, c in zip(tags[273], tags[279]))
    a = np.frombuffer(data, dt)
    if planar == 2:
        a = a[:spp * H * W].reshape(spp, H, W)
    else:
        a = a[:H * W * spp].reshape(H, W, spp).transpose(2, 0, 1)
    a = np.ascontiguousarray(a.astype(dt.newbyteorder("=")))
    return a[0] if spp == 1 else a


def _write_tiff(path, array):
    C, H, W = array.shape
    a = np.ascontiguousarray(array.astype(array.dtype.newbyteorder("<")))
    fmt = 3 if array.dtype.kind == "f" else 1
    bits = array.dtype.itemsize * 8
    plane = H * W * array.dtype.itemsize
    entries = []  # (tag, type, values)
    entries.append((256, 4, [W]))
    entries.append((257, 4, [H]))
    entries.append((258, 3, [bits] * C))
    entries.append((259, 3, [1]))
    entries.append((262, 3, [1]))
    entries.append((273, 4, None))  # strip offsets, patched below
    entries.append((277, 3, [C]))
    entries.append((278, 4, [H]))
    entries.append((279, 4, [plane] * C))
    entries.append((284, 3, [2]))   # planar: one strip per band
    if C > 1:
        entries.append((338, 3, [0] * (C - 1)))
    entries.append((339, 3, [fmt] * C))
    ifd_off = 8
    ifd_size = 2 + 12 * len(entries) + 4
    extra_off = ifd_off + ifd_size
    extra = b""
    data_off_holder = []

    def place(vals, typ):
        nonlocal extra
        size = 2 if typ == 3 else 4
        raw = struct.pack("<" + ("H" if typ == 3 else "I") * len(vals), *vals)
        if size * len(vals) <= 4:
            return raw.ljust(4, b"\0")
        off = extra_off + len(extra)
        extra += raw + (b"\0" if len(raw) % 2 else b"")
        return struct.pack("<I", off)

    # first pass to learn the size of the out-of-line area
    strip_slot = C * 4 if C * 4 > 4 else 0
    body = b""
    for tag, typ, vals in entries:
        if tag == 273:
            body += b"\0" * 12
            continue
        body += struct.pack("<HHI", tag, typ, len(vals)) + place(vals, typ)
    strip_tab_off = extra_off + len(extra)
    data_off = strip_tab_off + strip_slot
    data_off += data_off % 2
    offs = [data_off + i * plane for i in range(C)]
    extra2 = extra
    if strip_slot:
        strip_val = struct.pack("<I", strip_tab_off)
        extra2 += struct.pack("<%dI" % C, *offs)
    else:
        strip_val = struct.pack("<I", offs[0])
    out = struct.pack("<2sHI", b"II", 42, ifd_off) + struct.pack("<H", len(entries))
    for tag, typ, vals in entries:
        if tag == 273:
            out += struct.pack("<HHI", 273, 4, C) + strip_val
        else:
            start = 12 * [e[0] for e in entries].index(tag)
            out += body[start:start + 12]
    out += struct.pack("<I", 0) + extra2
    out = out.ljust(data_off, b"\0")
    with open(path, "wb") as f:
        f.write(out)
        f.write(a.tobytes())
