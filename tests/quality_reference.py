"""The reference of the quality report (lbdrn_hip.quality, csrc/quality.hip): int64 numpy for the integer fields, float64
numpy for SSIM and the spectral angle, the sums over windows and pixels by math.fsum (the exactly rounded sum).  Written from
the definitions in include/lbdrn_quality.h, sharing no code with the library.  TEST INFRASTRUCTURE."""
import math

import numpy as np

HIST_BINS = 257
TAPS, SIGMA = 11, 1.5


def weights():
    x = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    w = np.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return w / w.sum()


def band_stats(a, b):
    """a, b: [H,W] unsigned -> dict of Python integers"""
    e = a.astype(np.int64) - b.astype(np.int64)
    m = np.abs(e)
    hist = np.bincount(np.minimum(m, 256).ravel(), minlength=HIST_BINS)
    return {"n": int(e.size), "sse": int((m.astype(np.uint64) ** 2).sum(dtype=np.uint64)), "sae": int(m.sum()), "sum_err": int(e.sum()),
            "max_abs": int(m.max()), "hist": [int(v) for v in hist]}


def _blur(x, w):
    """the separable window over the positions where it lies wholly inside: [H,W] -> [H-10, W-10]"""
    ow, oh = x.shape[1] - TAPS + 1, x.shape[0] - TAPS + 1
    h = sum(w[k] * x[:, k:k + ow] for k in range(TAPS))
    return sum(w[k] * h[k:k + oh, :] for k in range(TAPS))


def ssim_map(a, b, peak):
    """[H,W] -> the SSIM of every window wholly inside, [H-10, W-10] float64; None where H < 11 or W < 11"""
    if a.shape[0] < TAPS or a.shape[1] < TAPS:
        return None
    a, b, w = a.astype(np.float64), b.astype(np.float64), weights()
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    ma, mb = _blur(a, w), _blur(b, w)
    va, vb, cov = _blur(a * a, w) - ma * ma, _blur(b * b, w) - mb * mb, _blur(a * b, w) - ma * mb
    return ((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


def sam_map(a, b):
    """a, b: [C,H,W] -> (theta [H,W] float64, undefined [H,W] bool)"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    C = a.shape[0]
    dot = (a * b).sum(axis=0)
    cross = np.zeros(a.shape[1:], np.float64)
    for i in range(C):
        for j in range(i + 1, C):
            d = (a[i] * b[j] - a[j] * b[i]).astype(np.float64)      # |d| < 2^33: exact
            cross += d * d
    za, zb = ~a.any(axis=0), ~b.any(axis=0)
    theta = np.arctan2(np.sqrt(cross), dot.astype(np.float64))
    theta[za & zb] = 0.0
    return theta, za ^ zb


def compare(a, b, peak=10000.0, ssim=True, sam=True):
    """-> {"bands": [dict per band], "sam_n", "sam_undefined", "sam_sum", "sam_max"}: the fields of the library's result"""
    a = a if a.ndim == 3 else a[None]
    b = b if b.ndim == 3 else b[None]
    assert a.shape == b.shape and a.dtype == b.dtype
    bands = []
    for c in range(a.shape[0]):
        rec = band_stats(a[c], b[c])
        m = ssim_map(a[c], b[c], peak) if ssim else None
        rec["ssim_n"] = 0 if m is None else int(m.size)
        rec["ssim_sum"] = 0.0 if m is None else math.fsum(m.ravel().tolist())
        bands.append(rec)
    out = {"bands": bands, "sam_n": 0, "sam_undefined": 0, "sam_sum": 0.0, "sam_max": 0.0}
    if sam and 2 <= a.shape[0] <= 16:
        theta, undefined = sam_map(a, b)
        good = theta[~undefined]
        out.update(sam_n=int(good.size), sam_undefined=int(undefined.sum()), sam_sum=math.fsum(good.tolist()),
                   sam_max=float(good.max()) if good.size else 0.0)
    return out
