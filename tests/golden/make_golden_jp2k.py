"""Writes tests/golden/jp2k_openjpeg.npz: a handful of small .jp2 files written by OpenJPEG (through
lbdrn_hip/jp2.py, i.e. liblbdrn_jp2.so) and the planes that went in, so that the JPEG 2000 oracle's decoder and parser
(oracle/jp2k_oracle.c) are checked against OpenJPEG's bytes where OpenJPEG itself is absent.

    python tests/golden/make_golden_jp2k.py

8 and 16 bits, one to three components, tiled and untiled, and one file with empty packets (a constant plane: every
high-pass packet is empty)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "lbdrn-msic_amd"))

from lbdrn_hip import jp2  # noqa: E402
from lbdrn_hip.synth import synthetic_tile  # noqa: E402


def cases():
    yield "u8_1x40x52", (synthetic_tile(0, 1, 40, 52) >> 8).astype(np.uint8)
    yield "u16_3x37x70", np.ascontiguousarray(synthetic_tile(1, 3, 37, 70) >> 5)
    yield "u8_3x64x65", (synthetic_tile(2, 3, 64, 65) >> 8).astype(np.uint8)
    yield "u16_2x1030x24_tiled", np.ascontiguousarray(synthetic_tile(3, 2, 1030, 24) >> 5)
    yield "u16_1x3x1100_tiled", np.ascontiguousarray(synthetic_tile(4, 1, 3, 1100) >> 5)
    yield "u16_1x70x70_constant_empty_packets", np.full((1, 70, 70), 1234, np.uint16)
    rng = np.random.default_rng(20261016)
    yield "u16_2x19x23_random", rng.integers(0, 65536, (2, 19, 23)).astype(np.uint16)


def main():
    out = {}
    for name, x in cases():
        f = jp2.encode(x)
        assert np.array_equal(jp2.decode(f), x)
        out["planes_" + name] = x
        out["file_" + name] = np.frombuffer(f, np.uint8)
    path = os.path.join(HERE, "jp2k_openjpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
