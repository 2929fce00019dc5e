"""Shared by tests/test_quality_host.py and tests/test_gpu_quality.py: the host build of the quality report's text
(tests/quality_host_shim.cpp, compiled by g++ into a temporary directory), the shapes and the data classes of the tests, the
reference results (tests/quality_reference.py, computed once per case) and the comparison under the derived tolerances.
TEST INFRASTRUCTURE."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import quality_reference as R  # noqa: E402

CSRC = os.path.join(ROOT, "lbdrn-msic_amd", "csrc")
BAND_WORDS, PIXEL_WORDS, HIST = 264, 4, 257
_shim = None

# Tolerances, derived: a moment's rounding error is at most about 64 eps v^2 and enters through
# sigma^2 / C2, so |delta SSIM| <~ 64 eps (1 + v^2 / C2) = 3.4e-10 at v = 65535, peak = 10000; per-pixel angles are a few
# eps off and a 20,000-term sequential sum is 7e-15 relative from the exact one.
SSIM_TOL = 1e-9          # absolute, on a band's mean SSIM
SAM_MEAN_RTOL = 1e-12
SAM_MAX_RTOL = 1e-14

STAT_ROWS, SSIM_TILE = 4, 32      # the library's cuts (quality_shim_stat_rows / quality_shim_ssim_tile say the same)

# (C, H, W): one sample, no window, one window, odd sizes, more than one block, 16 bands; then the SSIM tile's side - 1 / + 1 (31 and 33 windows a side) and the statistics pass's row
# chunk - 1 / + 1
SHAPES = ((1, 1, 1), (1, 10, 40), (1, 11, 11), (3, 12, 75), (8, 48, 80), (4, 65, 129), (16, 33, 70), (2, 200, 300),
          (1, SSIM_TILE + 10 - 1, SSIM_TILE + 10 + 1), (2, STAT_ROWS - 1, 20), (3, STAT_ROWS + 1, 9))
U8_SHAPES = ((3, 12, 75), (4, 65, 129), (16, 33, 70))
BIG_BAND_SHAPE = (2, 65, 64)      # holds a 64 x 64 band of 65535 against 0, and one row more: sse passes 2^32 and 2^44


def shape_id(s):
    return "x".join(str(v) for v in s)


def cxx():
    c = shutil.which(os.environ.get("CXX", "g++"))
    if c is None:
        pytest.skip("no host C++ compiler (g++): the report's host text cannot be compiled")
    return c


def load_shim(tmp_path_factory):
    global _shim
    if _shim is None:
        out = os.path.join(str(tmp_path_factory.mktemp("quality_shim")), "libquality_host_shim.so")
        subprocess.check_call([cxx(), "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", out,
                               os.path.join(ROOT, "tests", "quality_host_shim.cpp")])
        L = ctypes.CDLL(out)
        u64, i64, vp = ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p
        L.quality_shim_result_bytes.argtypes, L.quality_shim_result_bytes.restype = [ctypes.c_int], u64
        L.quality_shim_workspace.argtypes, L.quality_shim_workspace.restype = [ctypes.c_int] * 3 + [ctypes.c_uint32], u64
        L.quality_shim_weights.argtypes = [vp]
        L.quality_shim_compare.argtypes = [vp, i64, i64, vp, i64, i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_uint32, vp]
        _shim = L
    return _shim


def shim_compare(L, a, b, peak=10000.0, what=3):
    """the result words of the host build on two contiguous [C,H,W] arrays, the buffer guarded behind its stated size"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    C, H, W = a.shape
    n = L.quality_shim_result_bytes(C) // 8
    assert n == C * BAND_WORDS + PIXEL_WORDS
    out = np.full(n + 8, 0x7777777777777777, np.uint64)
    rc = L.quality_shim_compare(a.ctypes.data, W, H * W, b.ctypes.data, W, H * W, a.dtype.itemsize * 8, C, H, W, peak, what, out.ctypes.data)
    assert rc == 0
    assert (out[n:] == 0x7777777777777777).all(), "the host build wrote behind the result"
    return out[:n].copy()


# ---------------------------------------------------------------- data

def data_classes(shape, dtype=np.uint16, seed=11):
    """name -> (a, b) for one shape: identical rasters, noise in the low 5 bits, samples at the extremes, a flat raster one off,
    and pixels that are zero in every band of a, of b and of both"""
    C, H, W = shape
    top = 255 if np.dtype(dtype).itemsize == 1 else 65535
    rng = np.random.default_rng(seed + 1000 * C + 10 * H + W)
    a = rng.integers(0, top + 1, shape).astype(dtype)
    out = {"identical": (a, a.copy())}
    low = rng.integers(0, 32, shape).astype(dtype)
    out["low 5 bits redrawn"] = (a, ((a & ~dtype(31)) | low).astype(dtype))
    out["extremes"] = (rng.choice([0, top], shape).astype(dtype), rng.choice([0, top], shape).astype(dtype))
    out["flat top against top - 1"] = (np.full(shape, top, dtype), np.full(shape, top - 1, dtype))
    # all-zero pixels in a, in b and in both
    za, zb = a.copy(), rng.integers(0, top + 1, shape).astype(dtype)
    mask = rng.integers(0, 4, (H, W))
    za[:, mask == 1] = 0
    zb[:, mask == 2] = 0
    za[:, mask == 3] = 0
    zb[:, mask == 3] = 0
    out["zero pixels"] = (za, zb)
    return out


def big_band():
    C, H, W = BIG_BAND_SHAPE
    rng = np.random.default_rng(5)
    a = rng.integers(0, 65536, BIG_BAND_SHAPE).astype(np.uint16)
    b = a.copy()
    a[0] = 65535
    b[0] = 0
    assert 65 * 64 * 65535 ** 2 > 1 << 44
    return a, b


_refs = {}


def reference(key, a, b, peak, ssim=True, sam=True):
    """tests/quality_reference.py on (a, b), computed once per key and left unchanged"""
    k = (key, peak, ssim, sam)
    if k not in _refs:
        _refs[k] = R.compare(a, b, peak, ssim, sam)
    return _refs[k]


def peak_for(dtype, k=1):
    """the peaks the tolerance is derived for: 65535 or 10000 on 16-bit data (the data classes alternate; the flat raster, the
    worst case of the derivation, gets 10000), 255 on 8-bit data"""
    return 255.0 if np.dtype(dtype).itemsize == 1 else (65535.0, 10000.0)[k % 2]


# ---------------------------------------------------------------- comparison

def unpack(words, C):
    """result words -> the reference's dict layout"""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    assert w.size == C * BAND_WORDS + PIXEL_WORDS
    bands = []
    for c in range(C):
        r = w[c * BAND_WORDS:(c + 1) * BAND_WORDS]
        bands.append({"n": int(r[0]), "sse": int(r[1]), "sae": int(r[2]), "sum_err": int(r[3:4].view(np.int64)[0]), "max_abs": int(r[4]),
                      "hist": [int(v) for v in r[5:5 + HIST]], "ssim_n": int(r[5 + HIST]), "ssim_sum": float(r[6 + HIST:7 + HIST].view(np.float64)[0])})
    p = w[C * BAND_WORDS:]
    return {"bands": bands, "sam_n": int(p[0]), "sam_undefined": int(p[1]), "sam_sum": float(p[2:3].view(np.float64)[0]),
            "sam_max": float(p[3:4].view(np.float64)[0])}


def assert_matches(got, want, label="", report=None):
    """every field of a result against the reference: integers equal, the band's mean SSIM within SSIM_TOL, the mean angle
    within SAM_MEAN_RTOL and the largest within SAM_MAX_RTOL (both relative).  report: a dict that receives the largest
    distances seen"""
    assert len(got["bands"]) == len(want["bands"]), label
    for c, (g, w) in enumerate(zip(got["bands"], want["bands"])):
        for k in ("n", "sse", "sae", "sum_err", "max_abs", "hist", "ssim_n"):
            assert g[k] == w[k], (label, c, k, g[k] if k != "hist" else "hist", w[k] if k != "hist" else "")
        if w["ssim_n"]:
            d = abs(g["ssim_sum"] / g["ssim_n"] - w["ssim_sum"] / w["ssim_n"])
            if report is not None:
                report["ssim"] = max(report.get("ssim", 0.0), d)
            assert d <= SSIM_TOL, (label, c, "ssim", d)
        else:
            assert g["ssim_sum"] == 0.0, (label, c)
    for k in ("sam_n", "sam_undefined"):
        assert got[k] == want[k], (label, k, got[k], want[k])
    if want["sam_n"]:
        gm, wm = got["sam_sum"] / got["sam_n"], want["sam_sum"] / want["sam_n"]
        d = abs(gm - wm) / wm if wm else abs(gm)
        dm = abs(got["sam_max"] - want["sam_max"]) / want["sam_max"] if want["sam_max"] else abs(got["sam_max"])
        if report is not None:
            report["sam_mean"] = max(report.get("sam_mean", 0.0), d)
            report["sam_max"] = max(report.get("sam_max", 0.0), dm)
        assert d <= SAM_MEAN_RTOL, (label, "sam mean", d)
        assert dm <= SAM_MAX_RTOL, (label, "sam max", dm)
    else:
        assert got["sam_sum"] == 0.0 and got["sam_max"] == 0.0, label
