"""The overview levels of a raster, reduced on the GPU: the ctypes binding of liblbdrn_pyramid.so (include/lbdrn_pyramid.h,
csrc/pyramid.hip, csrc/pyramid.inc).  Built by csrc/build.py beside liblbdrn_quality.so; LBDRN_PYRAMID_LIB names another file.

    level_sizes(H, W, overviews, tile=None)   [(H_k, W_k)] of the levels 1 .. L: overviews "auto" (level k as long as the
                                              longer side of level k - 1 is above the tile's longer side), a count, or None
    build(tensor, levels, resampling="average", nodata=None, stream=None)
        tensor: [C,H,W] in HBM, uint8, or int16 / uint16 storage for 16-bit samples; a view with unit innermost stride is
        reduced where it lies.  Returns the levels 1 .. L as [C,H_k,W_k] tensors, views into one allocation.  Level k is
        computed from level k - 1: H_k = ceil(H_{k-1} / 2), W_k = ceil(W_{k-1} / 2).  "average": the mean of the 2 x 2 source
        samples that lie inside the level and differ from nodata, rounded half up, nodata where there is none; "nearest": the
        sample (2y, 2x).  No host sync.

    python -m lbdrn_hip.pyramid IN.tif OUT.tif [--overviews auto|N] [--resampling average|nearest] [--nodata V] [--tile N]
                                               [--no-georef]
        any TIFF this package reads -> a tiled, Deflate-compressed file with its overviews, read, reduced and written on the
        GPU; the georeferencing tags of IN are carried over."""
import ctypes

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
AVERAGE, NEAREST = 0, 1                                             # LBDRN_PYR_AVERAGE, LBDRN_PYR_NEAREST
RESAMPLINGS = {"average": AVERAGE, "nearest": NEAREST}
DEFAULT_TILE = 256                                                  # tiff_write.DEFAULT_TILE


class PyramidError(NativeError):
    pass


class Desc(ctypes.Structure):
    """lbdrn_pyr_desc"""
    _fields_ = [("C", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("bits", ctypes.c_int32),
                ("resampling", ctypes.c_int32), ("has_nodata", ctypes.c_int32), ("nodata", ctypes.c_uint32),
                ("reserved", ctypes.c_int32), ("row_pitch", ctypes.c_int64), ("plane_pitch", ctypes.c_int64)]


_i32, _vp, _sz, _dp, _ip = ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Desc), ctypes.POINTER(ctypes.c_int32)
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_pyramid.h
    "lbdrn_pyr_last_error": (ctypes.c_char_p, []),
    "lbdrn_pyr_abi_version": (ctypes.c_int, []),
    "lbdrn_pyr_level_count": (ctypes.c_int, [_i32, _i32, _i32]),
    "lbdrn_pyr_level_size": (ctypes.c_int, [_i32, _i32, _i32, _ip, _ip]),
    "lbdrn_pyr_level_offset": (_sz, [_dp, _i32]),
    "lbdrn_pyr_output_bytes": (_sz, [_dp, _i32]),
    "lbdrn_pyr_build": (ctypes.c_int, [_dp, _vp, _i32, _vp, _sz, _vp]),
}
_NATIVE = Library("liblbdrn_pyramid.so", "LBDRN_PYRAMID_LIB", "lbdrn_pyr_", ABI_VERSION, SIGNATURES, PyramidError)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


# ---------------------------------------------------------------- the levels of a raster (needs neither library nor device)

def _half(n):
    return (n + 1) // 2


def max_levels(H, W):
    """the levels a raster has: a level whose source is 1 x 1 does not exist"""
    k = 0
    while H > 1 or W > 1:
        H, W, k = _half(H), _half(W), k + 1
    return k


def _tile_side(tile):
    if tile is None:
        return DEFAULT_TILE
    if isinstance(tile, (tuple, list)):
        return max(int(tile[0]), int(tile[1]))
    return int(tile)


def parse_overviews(value):
    """"auto", None or a count >= 0, from the spelling of a command line or of a keyword; ValueError for anything else"""
    if value is None or value == "auto":
        return value
    try:
        n = int(value)
        if n >= 0 and (isinstance(value, str) or n == value) and not isinstance(value, bool):
            return n
    except (TypeError, ValueError):
        pass
    raise ValueError(f"overviews = {value!r}: 'auto' or a count of levels")


def level_sizes(H, W, overviews, tile=None):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"a {H} x {W} raster has no levels")
    overviews = parse_overviews(overviews)
    if overviews is None:
        return []
    if overviews == "auto":
        stop = _tile_side(tile)
        if stop < 1:
            raise ValueError(f"tile = {tile!r}: at least 1")
        n = 0
        h, w = H, W
        while max(h, w) > stop:
            h, w, n = _half(h), _half(w), n + 1
    else:
        n = overviews
        if n > max_levels(H, W):
            raise ValueError(f"overviews = {n}: a {H} x {W} raster has {max_levels(H, W)} levels (the source of a further one would be 1 x 1)")
    out = []
    for _ in range(n):
        H, W = _half(H), _half(W)
        out.append((H, W))
    return out


def check_options(resampling, nodata, bits=16):
    """(resampling code, has_nodata, nodata) or ValueError; needs no device"""
    if resampling not in RESAMPLINGS:
        raise ValueError(f"resampling = {resampling!r}: 'average' and 'nearest' are built")
    if nodata is None:
        return RESAMPLINGS[resampling], 0, 0
    if isinstance(nodata, bool) or int(nodata) != nodata or not 0 <= int(nodata) < (1 << bits):
        raise ValueError(f"nodata = {nodata!r}: a value the {bits}-bit samples can hold")
    return RESAMPLINGS[resampling], 1, int(nodata)


# ---------------------------------------------------------------- the call

def build(tensor, levels, resampling="average", nodata=None, stream=None):
    import torch
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 3 or tensor.dtype not in (torch.uint8, torch.int16, torch.uint16):
        raise ValueError("build takes a [C,H,W] tensor of uint8, or of int16 / uint16 holding unsigned 16-bit samples")
    C, H, W = (int(v) for v in tensor.shape)
    bits = 8 if tensor.dtype == torch.uint8 else 16
    code, has_nodata, nd = check_options(resampling, nodata, bits)
    levels = int(levels)
    if min(C, H, W) < 1:
        raise ValueError(f"an empty raster: {(C, H, W)}")
    if not 1 <= levels <= max_levels(H, W):
        raise ValueError(f"levels = {levels}: a {H} x {W} raster has 1 .. {max_levels(H, W)} (the source of a further one would be 1 x 1)")
    if not tensor.is_cuda:
        raise PyramidError("overviews are built on the GPU, where the planes lie; there is no CPU path in this package")
    t = tensor
    if t.stride(2) != 1 or t.stride(1) < W or t.stride(0) < 0:      # (the pitches the library takes)
        t = t.contiguous()
    L = lib()
    d = Desc(C, H, W, bits, code, has_nodata, nd, 0, t.stride(1), t.stride(0))
    nout = L.lbdrn_pyr_output_bytes(ctypes.byref(d), levels)
    if not nout:
        raise ValueError(f"geometry {C} x {H} x {W} is out of the library's range")
    dev = t.device
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = torch.empty(nout, dtype=torch.uint8, device=dev)
            _check(L.lbdrn_pyr_build(ctypes.byref(d), t.data_ptr(), levels, out.data_ptr(), nout, s.cuda_stream), "lbdrn_pyr_build")
    views = []
    for k, (h, w) in enumerate(level_sizes(H, W, levels), 1):
        at = L.lbdrn_pyr_level_offset(ctypes.byref(d), k)
        views.append(out[at:at + C * h * w * (bits // 8)].view(tensor.dtype).view(C, h, w))
    return views


# ---------------------------------------------------------------- the command line

def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m lbdrn_hip.pyramid",
                                description="rewrite a TIFF as a tiled, Deflate-compressed file with overviews, on the GPU")
    p.add_argument("src", metavar="IN.tif")
    p.add_argument("dst", metavar="OUT.tif")
    p.add_argument("--overviews", default="auto", metavar="auto|N", help="levels to write (default: until a level fits one tile)")
    p.add_argument("--resampling", default="average", choices=sorted(RESAMPLINGS))
    p.add_argument("--nodata", type=int, default=None, metavar="V", help="samples of this value do not enter an average")
    p.add_argument("--tile", type=int, default=None, metavar="N", help="tile side, a multiple of 16 (default 256)")
    p.add_argument("--no-georef", action="store_true", help="do not carry the georeferencing tags of IN over")
    args = p.parse_args(argv)
    try:
        overviews = parse_overviews(args.overviews)
    except ValueError as e:
        p.error(str(e))
    if args.nodata is not None and args.nodata < 0:
        p.error(f"--nodata {args.nodata}: a sample value")
    if args.tile is not None and (args.tile < 16 or args.tile % 16):
        p.error(f"--tile {args.tile}: a positive multiple of 16")
    if args.dst.endswith(".npy") or args.src.endswith(".npy"):
        p.error("IN and OUT are TIFF files")
    from . import raster_io
    geo = None if args.no_georef else raster_io.read_geo_tags(args.src)
    t = raster_io.read_raster_device(args.src)
    try:
        raster_io.write_raster_device(args.dst, t, compress="deflate", tile=args.tile, overviews=overviews, resampling=args.resampling,
                                      nodata=args.nodata, geo=geo or None)
    except ValueError as e:
        p.error(str(e))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
