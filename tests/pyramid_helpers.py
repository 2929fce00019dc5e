"""Shared by tests/test_pyramid_host.py and tests/test_gpu_pyramid.py: the host build of the overview pyramid's text
(tests/pyramid_host_shim.cpp, compiled by g++ into a temporary directory), the shapes, options and data classes of the tests,
the reference levels (tests/pyramid_reference.py, computed once per case and left unchanged), and whole pyramidal files put
together without a GPU from the host builds of the pyramid and of the TIFF writer.  TEST INFRASTRUCTURE."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import pyramid_reference as R  # noqa: E402
import tiff_write_helpers as TW  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
_shim = None

# (C, H, W): one output sample from two, a row, the worked example of the definition, odd sizes, more than one workgroup, one
# side reaching 1 while the other goes on, a power of two, and a width that is one more than a multiple of every vector
SHAPES = ((1, 1, 2), (1, 2, 1), (1, 1, 200), (1, 3, 3), (2, 37, 53), (8, 75, 130), (3, 5, 130), (1, 64, 64), (1, 65, 129))
RESAMPLINGS = ("average", "nearest")
DATA = ("random", "all maximum", "all nodata")
EXAMPLE = np.array([[[0, 1, 65535], [2, 3, 65535], [65535, 65535, 65534]]], np.uint16)
EXAMPLE_LEVEL = np.array([[[2, 65535], [65535, 65534]]], np.uint16)


def shape_id(s):
    return "x".join(str(v) for v in s)


def top_of(dtype):
    return 255 if np.dtype(dtype).itemsize == 1 else 65535


def nodatas(dtype):
    """absent, 0 and the largest sample"""
    return (None, 0, top_of(dtype))


def raster(shape, dtype, data, nodata, seed=23):
    """random: every value, with a third of the samples at 0 and a fifth at the maximum, so that with either as nodata a
    footprint holds 0 .. 4 valid samples; all maximum: sums that need more than 16 bits; all nodata: no valid sample anywhere
    (the maximum where nodata is absent)"""
    top = top_of(dtype)
    if data == "all maximum":
        return np.full(shape, top, dtype)
    if data == "all nodata":
        return np.full(shape, top if nodata is None else nodata, dtype)
    if shape == EXAMPLE.shape and np.dtype(dtype) == np.uint16:
        return EXAMPLE.copy()
    rng = np.random.default_rng(seed + 1000 * shape[0] + 10 * shape[1] + shape[2])
    a = rng.integers(0, top + 1, shape).astype(dtype)
    kind = rng.integers(0, 15, shape)
    a[kind < 5] = 0
    a[kind >= 12] = top
    return a


_refs = {}


def reference(a, key, resampling, nodata):
    """every level of `a`, computed once per key and left unchanged"""
    k = (key, resampling, nodata)
    if k not in _refs:
        levels = R.pyramid(a, R.max_levels(*a.shape[1:]), resampling, nodata)
        for lv in levels:
            lv.setflags(write=False)
        _refs[k] = levels
    return _refs[k]


def cases(shape):
    """(dtype, resampling, nodata, data name, raster, reference levels) of one shape"""
    for dtype in (np.uint8, np.uint16):
        for nodata in nodatas(dtype):
            for data in DATA:
                a = raster(shape, dtype, data, nodata)
                for resampling in RESAMPLINGS:
                    yield dtype, resampling, nodata, data, a, reference(a, (shape, np.dtype(dtype).name, data, nodata), resampling, nodata)


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        out = os.path.join(str(tmp_path_factory.mktemp("pyramid_shim")), "libpyramid_host_shim.so")
        subprocess.check_call([TW.cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                               os.path.join(ROOT, "tests", "pyramid_host_shim.cpp")])
        L = ctypes.CDLL(out)
        i, u64, i64, vp = ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p
        L.pyr_shim_max_levels.argtypes = [i, i]
        L.pyr_shim_level_count.argtypes = [i, i, i]
        L.pyr_shim_level_size.argtypes, L.pyr_shim_level_size.restype = [i, i, i, ctypes.POINTER(i), ctypes.POINTER(i)], None
        L.pyr_shim_level_offset.argtypes, L.pyr_shim_level_offset.restype = [i] * 5, u64
        L.pyr_shim_output_bytes.argtypes, L.pyr_shim_output_bytes.restype = [i] * 5, u64
        L.pyr_shim_rounded_mean.argtypes, L.pyr_shim_rounded_mean.restype = [ctypes.c_uint32] * 2, ctypes.c_uint32
        L.pyr_shim_build.argtypes = [vp, i64, i64, i, i, i, i, i, i, ctypes.c_uint32, i, vp]
        _shim = L
    return _shim


def split_levels(L, raw, C, H, W, levels, dtype):
    """the levels of an output buffer of the library's layout, as arrays"""
    sb = np.dtype(dtype).itemsize
    out = []
    for k, (h, w) in enumerate(R.level_sizes(H, W, levels), 1):
        at = L.pyr_shim_level_offset(C, H, W, k, sb)
        assert at % 256 == 0
        out.append(raw[at:at + C * h * w * sb].view(dtype).reshape(C, h, w).copy())
    return out


def shim_build(L, a, levels, resampling="average", nodata=None, view=None):
    """the levels 1 .. `levels` by the host build.  a: a contiguous [C,H,W] array; view = (y0, x0, h, w): reduce that window of
    it where it lies.  The output is a buffer of exactly output_bytes with a guard behind it; the padding between two levels
    must come back untouched."""
    a = np.ascontiguousarray(a)
    C, Hh, Ww = a.shape
    y0, x0, h, w = view if view is not None else (0, 0, Hh, Ww)
    sb = a.dtype.itemsize
    n = L.pyr_shim_output_bytes(C, h, w, levels, sb)
    out = np.full(n + 64, 0x77, np.uint8)
    rc = L.pyr_shim_build(a.ctypes.data + (y0 * Ww + x0) * sb, Ww, Hh * Ww, 8 * sb, C, h, w, R_CODE[resampling], nodata is not None,
                          0 if nodata is None else nodata, levels, out.ctypes.data)
    assert rc == 0
    assert (out[n:] == 0x77).all(), "the host build wrote behind the output"
    got = split_levels(L, out, C, h, w, levels, a.dtype)
    used = np.zeros(n, bool)
    for k, lv in enumerate(got, 1):
        at = L.pyr_shim_level_offset(C, h, w, k, sb)
        used[at:at + lv.nbytes] = True
    assert (out[:n][~used] == 0x77).all(), "the host build wrote into the padding between two levels"
    return got


R_CODE = {"average": 0, "nearest": 1}


# ---------------------------------------------------------------- georeferencing tags

# one value for each tag the package carries: (tag, type, count, little-endian value bytes), ascending
GEO = [
    (33550, 12, 3, np.array([10.0, 10.0, 0.0], "<f8").tobytes()),                              # ModelPixelScale
    (33922, 12, 6, np.array([0.0, 0.0, 0.0, 399960.0, 5700000.5, 0.0], "<f8").tobytes()),      # ModelTiepoint
    (34264, 12, 16, np.arange(16, dtype="<f8").tobytes()),                                     # ModelTransformation
    (34735, 3, 16, np.array([1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32632], "<u2").tobytes()),      # GeoKeyDirectory
    (34736, 12, 2, np.array([6378137.0, 298.257223563], "<f8").tobytes()),                     # GeoDoubleParams
    (34737, 2, 22, b"WGS 84 / UTM zone 32N|"),                                                 # GeoAsciiParams
    (42112, 2, 27, b"<GDALMetadata>\n</GDALMetadata>"[:26] + b"\0"),                           # GDAL_METADATA
    (42113, 2, 2, b"0\0"),                                                                     # GDAL_NODATA
]
_GEO_ELEMENT = {2: 1, 3: 2, 12: 8}


def with_tags(buf, geo):
    """a classic TIFF of one IFD, either byte order, with the tags of `geo` added to it: the IFD is written again, with the
    new entries, behind the file's end and the header points there; the values go in the file's byte order"""
    import struct
    bo = {b"II": "<", b"MM": ">"}[bytes(buf[:2])]
    assert struct.unpack_from(bo + "H", buf, 2)[0] == 42
    off = struct.unpack_from(bo + "I", buf, 4)[0]
    n = struct.unpack_from(bo + "H", buf, off)[0]
    entries = [(struct.unpack_from(bo + "H", buf, off + 2 + 12 * i)[0], bytes(buf[off + 2 + 12 * i:off + 14 + 12 * i])) for i in range(n)]
    out = bytearray(buf) + b"\0" * (len(buf) & 1)
    ifd_at = len(out)
    at = ifd_at + 2 + 12 * (n + len(geo)) + 4
    extra = bytearray()
    for tag, typ, cnt, raw in geo:
        size = _GEO_ELEMENT[typ]
        raw = np.frombuffer(raw, "<u%d" % size).astype(bo + "u%d" % size).tobytes()
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            field = struct.pack(bo + "I", at + len(extra))
            extra += raw + b"\0" * (len(raw) & 1)
        entries.append((tag, struct.pack(bo + "HHI", tag, typ, cnt) + field))
    entries.sort(key=lambda e: e[0])
    out += struct.pack(bo + "H", len(entries)) + b"".join(e[1] for e in entries) + struct.pack(bo + "I", 0) + extra
    struct.pack_into(bo + "I", out, 4, ifd_at)
    return bytes(out)


# ---------------------------------------------------------------- whole files without a GPU

def host_write(pyr_shim, tiffw_shim, a, tile=16, overviews="auto", resampling="average", nodata=None, geo=None, planar=2,
               compress="deflate"):
    """the bytes tiff_write.write_device writes, with both device stages done by their host builds"""
    from lbdrn_hip import pyramid, tiff_write
    C, H, W = a.shape
    bits = a.dtype.itemsize * 8
    cap = tiffw_shim.tiffw_shim_cap(8 if compress == "deflate" else 1)
    sizes = tiff_write.check_pyramid_options(H, W, bits, tile, None, overviews, resampling, nodata, geo)
    assert sizes == pyramid.level_sizes(H, W, overviews, tile)
    lays = [tiff_write.make_layout(C, h, w, bits, compress, tile, None, planar, None, cap=cap) for h, w in [(H, W)] + sizes]
    planes = [a] + (shim_build(pyr_shim, a, len(sizes), resampling, nodata) if sizes else [])
    bodies, counts = [], []
    for p, lay in zip(planes, lays):
        body, _, cnt = TW.host_encode(tiffw_shim, p, lay)
        bodies.append(body.tobytes())
        counts.append(cnt)
    head, offsets = tiff_write.assemble_pyramid(lays, counts, geo)
    return head + b"".join(reversed(bodies)), lays, offsets, counts
