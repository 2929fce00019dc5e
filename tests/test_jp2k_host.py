"""The GPU JPEG 2000 encoder's host side (base codec "jp2-gpu", csrc/jp2k.hip + jp2k_t2.inc), checked without a GPU: the
code-block geometry against an enumeration written here, the output bound, and the codec name through the Python layers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))

GEOMETRIES = [(1, 1), (1, 200), (33, 70), (300, 517), (1024, 1024), (1025, 64), (1029, 1061), (2048, 2048), (6000, 6000),
              (7550, 7550), (64, 64), (65, 129), (2, 2), (1024, 1025), (3000, 1)]


def _ceil_div(a, b):
    return -((-a) // b)


def block_count(C, H, W):
    """tiles -> components -> resolutions -> subbands -> the 64 x 64 grid anchored at 0 in subband coordinates (T.800 B.5,
    B.7); resolutions by the rule of csrc/jp2_shim.c; an empty subband has no block."""
    m, R = min(H, W), 1
    while (m >> R) > 0 and R < 6:
        R += 1
    tiled = H > 1024 or W > 1024
    tw, th = (1024, 1024) if tiled else (W, H)
    total = 0
    for ty0 in range(0, H, th):
        for tx0 in range(0, W, tw):
            tx1, ty1 = min(tx0 + tw, W), min(ty0 + th, H)
            per_component = 0
            for r in range(R):
                bands = [(R - 1, 0, 0)] if r == 0 else [(R - r, 1, 0), (R - r, 0, 1), (R - r, 1, 1)]
                for nb, xo, yo in bands:
                    half = (1 << (nb - 1)) if nb else 0
                    bx0, bx1 = _ceil_div(tx0 - half * xo, 1 << nb), _ceil_div(tx1 - half * xo, 1 << nb)
                    by0, by1 = _ceil_div(ty0 - half * yo, 1 << nb), _ceil_div(ty1 - half * yo, 1 << nb)
                    if bx1 > bx0 and by1 > by0:
                        per_component += (_ceil_div(bx1, 64) - bx0 // 64) * (_ceil_div(by1, 64) - by0 // 64)
            total += C * per_component
    return total


def _lib():
    from lbdrn_hip import _lib
    return _lib.lib()


def test_block_count_equals_an_independent_enumeration():
    L = _lib()
    assert block_count(8, 2048, 2048) == 32 * 259 == 8288
    for H, W in GEOMETRIES:
        for C in (1, 3, 8):
            assert L.lbdrn_jp2k_block_count(C, H, W) == block_count(C, H, W), (C, H, W)
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 5, 5), (1, 40000, 5)):
        assert L.lbdrn_jp2k_block_count(*bad) == 0
        assert L.lbdrn_jp2k_bound(*bad) == 0 and L.lbdrn_jp2k_workspace(*bad) == 0


def test_bound_is_monotone_and_covers_incompressible_planes():
    L = _lib()
    sizes = [1, 2, 63, 64, 65, 257, 300, 1024, 1025, 1100, 2048]
    for C in (1, 2, 5):
        for k, a in enumerate(sizes):
            for b in sizes[k + 1:]:
                assert L.lbdrn_jp2k_bound(C, a, 70) <= L.lbdrn_jp2k_bound(C, b, 70), (C, a, b)
                assert L.lbdrn_jp2k_bound(C, 70, a) <= L.lbdrn_jp2k_bound(C, 70, b), (C, a, b)
                assert L.lbdrn_jp2k_bound(C, a, a) <= L.lbdrn_jp2k_bound(C, b, b), (C, a, b)
    for H, W in GEOMETRIES:
        assert L.lbdrn_jp2k_bound(1, H, W) <= L.lbdrn_jp2k_bound(2, H, W) <= L.lbdrn_jp2k_bound(3, H, W)
        assert L.lbdrn_jp2k_bound(1, H, W) > 2 * H * W      # above the raw size of 16-bit planes
    from lbdrn_hip import jp2
    if jp2.available():
        x = np.random.default_rng(20260101).integers(0, 65536, (2, 257, 300)).astype(np.uint16)
        n = len(jp2.encode(x))
        assert n > x.nbytes                      # OpenJPEG's stream is larger than the raw planes (7 % here)
        assert L.lbdrn_jp2k_bound(2, 257, 300) >= n


def test_codec_name_is_accepted_and_unknown_names_are_refused(monkeypatch, tmp_path):
    from lbdrn_hip import container
    for name in ("jp2-gpu", "JP2-GPU", "jp2", "LBB2", "LBB1"):
        assert container.check_base_codec(name) == name
    for name in ("jp2-cpu", "nope", ""):
        with pytest.raises(ValueError, match="unknown MSB payload codec"):
            container.check_base_codec(name)
        with pytest.raises(ValueError, match="unknown MSB payload codec"):
            container.encode_base(np.zeros((1, 4, 4), np.uint16), codec=name)
    import torch
    if not torch.cuda.is_available():   # the name is known: what fails without a GPU is the device, loudly
        with pytest.raises(Exception) as e:
            container.encode_base(np.zeros((1, 4, 4), np.uint16), codec="jp2-gpu")
        assert not isinstance(e.value, ValueError)
    # encode.py: LBDRN_BASE_CODEC is read at import; main() refuses an unknown name before any work
    import importlib
    monkeypatch.setenv("LBDRN_BASE_CODEC", "jp2-gpu")
    sys.modules.pop("encode", None)
    enc = importlib.import_module("encode")
    assert enc.BASE_CODEC == "jp2-gpu"
    container.check_base_codec(enc.BASE_CODEC)
    monkeypatch.setenv("LBDRN_BASE_CODEC", "jp3")
    sys.modules.pop("encode", None)
    enc = importlib.import_module("encode")
    with pytest.raises(SystemExit):
        enc.main(["-i", str(tmp_path / "missing.tif"), "-o", str(tmp_path / "out")])
    sys.modules.pop("encode", None)
