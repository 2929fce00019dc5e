"""The overview pyramid in plain numpy, written from its definition (include/lbdrn_pyramid.h) and not
from csrc/pyramid.inc: the reference of tests/test_pyramid_host.py and tests/test_gpu_pyramid.py.

Level k has ceil(H_{k-1} / 2) x ceil(W_{k-1} / 2) samples and is computed from level k - 1.  average: output (y, x) is the mean,
rounded half up in integers, of the source samples (2y + dy, 2x + dx) that lie inside the level and (with nodata) differ from
nodata; nodata where there is none.  nearest: the sample (2y, 2x).  TEST INFRASTRUCTURE."""
import numpy as np


def half(n):
    return -(-n // 2)


def max_levels(H, W):
    k = 0
    while (H, W) != (1, 1):
        H, W, k = half(H), half(W), k + 1
    return k


def level_sizes(H, W, overviews, tile=256):
    """[(H_k, W_k)] for k = 1 .. L: overviews "auto" writes level k as long as max(H_{k-1}, W_{k-1}) > the tile's longer side"""
    stop = max(tile) if isinstance(tile, (tuple, list)) else tile
    out = []
    while (max(H, W) > stop) if overviews == "auto" else (len(out) < overviews):
        if (H, W) == (1, 1):
            raise ValueError("a level whose source is 1 x 1")
        H, W = half(H), half(W)
        out.append((H, W))
    return out


def reduce_level(a, resampling="average", nodata=None):
    """one level from the one before it: a is [C,H,W], uint8 or uint16"""
    C, H, W = a.shape
    if resampling == "nearest":
        return a[:, ::2, ::2].copy()
    assert resampling == "average"
    H2, W2 = half(H), half(W)
    v = np.zeros((C, 2 * H2, 2 * W2), np.int64)
    ok = np.zeros((C, 2 * H2, 2 * W2), bool)
    v[:, :H, :W] = a
    ok[:, :H, :W] = True if nodata is None else (a != nodata)
    v = np.where(ok, v, 0)
    s = v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
    n = ok[:, 0::2, 0::2].astype(np.int64) + ok[:, 0::2, 1::2] + ok[:, 1::2, 0::2] + ok[:, 1::2, 1::2]
    out = np.where(n > 0, (s + n // 2) // np.maximum(n, 1), -1 if nodata is None else nodata)
    assert out.min() >= 0
    return out.astype(a.dtype)


def pyramid(a, levels, resampling="average", nodata=None):
    """the levels 1 .. `levels` of a ([C,H,W]), each from the one before it"""
    out = []
    for _ in range(levels):
        if a.shape[1:] == (1, 1):
            raise ValueError("a level whose source is 1 x 1")
        a = reduce_level(a, resampling, nodata)
        out.append(a)
    return out
