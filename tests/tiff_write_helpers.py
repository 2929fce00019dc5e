"""Shared by tests/test_tiff_write_host.py and tests/test_gpu_tiff_write.py: the host build of the TIFF writer's format text
(tests/tiff_write_host_shim.cpp, compiled by g++ into a temporary directory), the device stage of lbdrn_hip.tiff_write done
with it, a reader made of lbdrn_hip.tiff.parse and tests/tiff_reference.py, and the rasters and segments the tests use.
TEST INFRASTRUCTURE."""
import ctypes
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tiff_reference as R  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
_shim = None

SEGMENTATIONS = (dict(rows_per_strip=1), dict(rows_per_strip=8), dict(rows_per_strip=37), dict(tile=(16, 16)), dict(tile=(32, 16)))
CODINGS = (("none", 1), ("deflate", 1), ("deflate", 2))      # (compress, predictor)

# The writer against zlib level 1 on the two golden rasters (planar, predictor 2, one tile a plane), as first recorded in
# DESIGN.md section 7 and profiles/tiff_write_timing.txt; the tests hold it to that ratio plus 0.02.
GOLDEN_SETUPS = (("rasters_learn_bands4.npz", 256, 1.1064), ("rasters_learn_bc64.npz", 128, 1.1021))


def base_raster(C=8, H=37, W=53, dtype=np.uint16, seed=5):
    """the generator of tests/test_tiff_host.py"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.integers(-60, 61, (C, H, W)), axis=2) + rng.integers(0, 65536, (C, H, 1))
    a[:, 3, :] = rng.integers(0, 65536, (C, W))      # a row of noise
    a[:, 7:9, :] = 513                               # two constant rows
    return (a % (256 if np.dtype(dtype).itemsize == 1 else 65536)).astype(dtype)


def cxx():
    c = shutil.which(os.environ.get("CXX", "g++"))
    if c is None:
        pytest.skip("no host C++ compiler (g++): the writer's host text cannot be compiled")
    return c


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        out = os.path.join(str(tmp_path_factory.mktemp("tiffw_shim")), "libtiff_write_host_shim.so")
        subprocess.check_call([cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                               os.path.join(ROOT, "tests", "tiff_write_host_shim.cpp")])
        L = ctypes.CDLL(out)
        u64, vp, sz = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t
        L.tiffw_shim_bound.argtypes, L.tiffw_shim_bound.restype = [u64], u64
        L.tiffw_shim_cap.argtypes, L.tiffw_shim_cap.restype = [ctypes.c_int], u64
        L.tiffw_shim_block_tokens.restype = ctypes.c_uint32
        L.tiffw_shim_adler32.argtypes, L.tiffw_shim_adler32.restype = [ctypes.c_char_p, sz], ctypes.c_uint32
        L.tiffw_shim_deflate.argtypes, L.tiffw_shim_deflate.restype = [ctypes.c_char_p, sz, vp, sz, vp, ctypes.c_int], u64
        L.tiffw_shim_lengths.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.tiffw_shim_rle.argtypes, L.tiffw_shim_rle.restype = [vp, ctypes.c_int, vp, ctypes.c_int, vp], ctypes.c_uint32
        L.tiffw_shim_segment_count.argtypes, L.tiffw_shim_segment_count.restype = [vp], ctypes.c_int64
        L.tiffw_shim_expected.argtypes, L.tiffw_shim_expected.restype = [vp, ctypes.c_int64], ctypes.c_int64
        L.tiffw_shim_gather.argtypes = [vp, vp, ctypes.c_int64, vp]
        _shim = L
    return _shim


def shim_deflate(L, data, fill=0xA5):
    """(zlib stream, [blocks, tokens, kinds, stored blocks]) of one segment through the host build; the output buffer is
    bound(n) bytes with 64 guard bytes behind it"""
    data = bytes(data)
    cap = L.tiffw_shim_bound(len(data))
    out = np.full(cap + 64, 0x77, np.uint8)
    stats = (ctypes.c_uint32 * 4)()
    n = L.tiffw_shim_deflate(data, len(data), out.ctypes.data, cap, stats, fill)
    assert n <= cap, f"{n} bytes from {len(data)}: above the bound of {cap}"
    assert (out[cap:] == 0x77).all(), "the encoder wrote behind its bound"
    return out[:n].tobytes(), list(stats)


def shim_gather(L, a, lay):
    """the uncompressed byte image of every segment of a ([C,H,W]) under lay, by the host build of the gather"""
    a = np.ascontiguousarray(a)
    nseg = L.tiffw_shim_segment_count(ctypes.byref(lay))
    assert nseg > 0
    segs = []
    for s in range(nseg):
        n = L.tiffw_shim_expected(ctypes.byref(lay), s)
        buf = np.full(n + 16, 0x77, np.uint8)
        assert L.tiffw_shim_gather(ctypes.byref(lay), a.ctypes.data, s, buf.ctypes.data) == 0
        assert (buf[n:] == 0x77).all(), "the gather wrote behind the segment"
        segs.append(buf[:n].tobytes())
    return segs


def host_encode(L, a, lay, stage=None):
    """what tiff_write.encode_device returns, from the host build: (body, offsets, counts).  stage: a dict that receives the
    segments after the gather ("raw") and after Deflate ("coded")"""
    raw = shim_gather(L, a, lay)
    coded = [shim_deflate(L, r)[0] for r in raw] if lay.compression == 8 else raw
    if stage is not None:
        stage["raw"], stage["coded"] = raw, coded
    counts = np.array([len(c) for c in coded], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(coded), np.uint8), offsets, counts


def reference_read(buf):
    """a whole file: lbdrn_hip.tiff's parser, the reference's segment decoders (zlib for Deflate) and placement -> [C,H,W]"""
    from lbdrn_hip import tiff
    sc = tiff.parse(buf)
    lay = sc.layout
    spp = 1 if lay.planar == 2 else lay.C
    segs = []
    for i, (o, n) in enumerate(zip(sc.offsets.tolist(), sc.counts.tolist())):
        rows = lay.seg_h if lay.tiled else min(lay.seg_h, lay.H - (i % -(-lay.H // lay.seg_h)) * lay.seg_h)
        segs.append(R.decompress(bytes(buf[o:o + n]), lay.compression, rows * lay.seg_w * spp * lay.bits // 8))
    return R.place_segments(segs, lay.C, lay.H, lay.W, np.uint8 if lay.bits == 8 else np.uint16,
                            tile=(lay.seg_w, lay.seg_h) if lay.tiled else None, rows_per_strip=lay.seg_h, planar=lay.planar,
                            predictor=lay.predictor, byteorder="<")


def huffman_only(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return c.compress(data) + c.flush()


def no_repeats(n, rng, alphabet=256):
    """n bytes in which no group of three bytes occurs twice: nothing for a match finder to find"""
    seen, out = set(), bytearray()
    while len(out) < n:
        b = int(rng.integers(0, alphabet))
        if len(out) >= 2:
            t = (out[-2], out[-1], b)
            if t in seen:
                continue
            seen.add(t)
        out.append(b)
    return bytes(out)


def special_segments(block_tokens):
    """name -> bytes: the encoder's hard cases"""
    rng = np.random.default_rng(17)
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()      # noqa: E731
    block = noise(32768)
    out = {f"{n} bytes": noise(n) for n in (1, 2, 3, 4)}
    out["constant 128 KiB"] = b"\x07" * 131072
    out["32 KiB of noise three times"] = block * 3
    out["128 KiB of noise"] = noise(131072)
    # one token more than a block holds: bytes without a repeated three-byte group are literals, one each
    out["one token more than a block"] = no_repeats(block_tokens + 1, rng, 32)
    out["literals only"] = no_repeats(2000, rng, 20)      # few symbols: a dynamic block, and no distance code in it
    out["one distance"] = bytes(i % 5 for i in range(6000))
    out["zero run of 138"] = bytes(rng.choice([10, 149], 6000).astype(np.uint8))
    out["zero run of 139"] = bytes(rng.choice([10, 150], 6000).astype(np.uint8))
    out["0xFF over 5552 bytes"] = b"\xff" * 70000
    return out


def golden_planes(name):
    img = np.load(os.path.join(GOLDEN, name))["img"]
    assert img.dtype == np.uint16
    return np.ascontiguousarray(img)
