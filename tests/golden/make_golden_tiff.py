"""Writes tests/golden/tiff_libtiff.npz: TIFF files written by libtiff (through Pillow) as byte arrays beside their pixels,
for the tests of the TIFF reader (tests/test_tiff_host.py, tests/test_gpu_tiff.py).  Needs Pillow built with libtiff; the
tests need neither.  TEST INFRASTRUCTURE.

    python tests/golden/make_golden_tiff.py

Files (key "<name>__file" uint8; the pixels [C,H,W] of all files of one family under "<family>__pixels", the family being the
name up to its first underscore):
    i16_* / rgb_*      I;16 and RGB at 37 x 53, compression tiff_lzw, tiff_adobe_deflate, packbits, raw, each with the
                       Predictor tag 1 and 2.  libtiff knows the predictor with LZW and Deflate only: with packbits and raw it
                       writes the tag and leaves the samples as they are -- and ignores the tag when it reads.
    strips64_lzw       300 x 400, 16 bit, LZW, RowsPerStrip = 64
    planar3_*          three 16-bit bands, PlanarConfiguration 2, assembled by tests/tiff_reference.py's writer from the strips
                       libtiff wrote for each band alone (Pillow writes no such mode itself)
    chunky4_lzw        four 16-bit bands, chunky, predictor 1: the strips libtiff wrote for a single band of 4 W columns

It also checks the other direction and stops if it fails: libtiff reads what tests/tiff_reference.py's LZW encoder and
its Deflate and PackBits writers produce (240 KB of smooth and 25 KB of noise samples, strips and tiles)."""
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tiff_reference as R  # noqa: E402


def smooth(rng, shape, step, bits):
    a = np.cumsum(rng.integers(-step, step + 1, shape), axis=-1) + rng.integers(0, 1 << bits, shape[:-1])[..., None]
    return (a % (1 << bits)).astype(np.uint16 if bits == 16 else np.uint8)


def libtiff_file(arr2d_or_rgb, compression, predictor=1, rows_per_strip=None):
    bio = io.BytesIO()
    info = {}
    if predictor != 1:
        info[317] = predictor
    if rows_per_strip:
        info[278] = rows_per_strip
    Image.fromarray(arr2d_or_rgb).save(bio, format="TIFF", compression=compression, tiffinfo=info)
    return bio.getvalue()


def strips_of(data):
    """(offsets, counts, RowsPerStrip) of a classic little-endian strip file, read with struct alone"""
    import struct
    assert data[:4] == b"II*\0"
    off = struct.unpack_from("<I", data, 4)[0]
    tags = {}
    for i in range(struct.unpack_from("<H", data, off)[0]):
        tag, typ, cnt, val = struct.unpack_from("<HHII", data, off + 2 + 12 * i)
        size = {3: 2, 4: 4}.get(typ)
        if size is None:
            continue
        at = off + 2 + 12 * i + 8 if size * cnt <= 4 else val
        tags[tag] = list(struct.unpack_from("<" + {2: "H", 4: "I"}[size] * cnt, data, at))
    return tags[273], tags[279], tags[278][0]


def main():
    assert features.check("libtiff"), "Pillow without libtiff"
    rng = np.random.default_rng(20240611)
    out = {}
    i16 = smooth(rng, (1, 37, 53), 40, 16)
    i16[0, 5, :20] = rng.integers(0, 65536, 20)
    rgb = smooth(rng, (3, 37, 53), 9, 8)
    for comp, short in (("tiff_lzw", "lzw"), ("tiff_adobe_deflate", "deflate"), ("packbits", "packbits"), ("raw", "raw")):
        for pred in (1, 2):
            out[f"i16_{short}_p{pred}__file"] = np.frombuffer(libtiff_file(i16[0], comp, pred), np.uint8)
            out[f"rgb_{short}_p{pred}__file"] = np.frombuffer(libtiff_file(np.ascontiguousarray(rgb.transpose(1, 2, 0)), comp, pred), np.uint8)
    out["i16__pixels"], out["rgb__pixels"] = i16, rgb
    # (plateaus of 5 x 3 samples on two ramps: the file and its pixels stay small in the archive)
    big = (((np.arange(400)[None, :] // 5) * 1301 + (np.arange(300)[:, None] // 3) * 1787) % 65536).astype(np.uint16)[None]
    f = libtiff_file(big[0], "tiff_lzw", 1, rows_per_strip=64)
    assert strips_of(f)[2] == 64, strips_of(f)[2]
    out["strips64_lzw__file"], out["strips64__pixels"] = np.frombuffer(f, np.uint8), big
    # planar multi-band: libtiff's own strips of each band, under an IFD written by the independent writer
    bands = smooth(rng, (3, 37, 53), 25, 16)
    for comp, short, code in (("tiff_lzw", "lzw", R.COMP_LZW), ("tiff_adobe_deflate", "deflate", R.COMP_DEFLATE)):
        strips, rps = [], None
        for b in range(3):
            f = libtiff_file(bands[b], comp, 2)
            offs, cnts, rps = strips_of(f)
            strips += [f[o:o + c] for o, c in zip(offs, cnts)]
        f, _ = R.write_tiff(bands, rows_per_strip=rps, planar=2, predictor=2, compression=code, segment_hook=lambda i, p: strips[i])
        out[f"planar3_{short}__file"], out["planar3__pixels"] = np.frombuffer(f, np.uint8), bands
    # chunky multi-band, predictor 1: a single band of 4 W columns is the same bytes
    chunky = smooth(rng, (4, 37, 53), 25, 16)
    wide = np.ascontiguousarray(chunky.transpose(1, 2, 0)).reshape(37, 53 * 4)
    f = libtiff_file(wide, "tiff_lzw", 1)
    offs, cnts, rps = strips_of(f)
    strips = [f[o:o + c] for o, c in zip(offs, cnts)]
    f, _ = R.write_tiff(chunky, rows_per_strip=rps, planar=1, predictor=1, compression=R.COMP_LZW, segment_hook=lambda i, p: strips[i])
    out["chunky4_lzw__file"], out["chunky4__pixels"] = np.frombuffer(f, np.uint8), chunky

    # the other direction: libtiff reads the reference writers
    smooth_big = smooth(rng, (1, 300, 400), 30, 16)                      # 240 KB
    noise = rng.integers(0, 65536, (1, 64, 200)).astype(np.uint16)      # 25.6 KB
    n = 0
    for a in (smooth_big, noise):
        for comp in (R.COMP_LZW, R.COMP_DEFLATE, R.COMP_DEFLATE_OLD, R.COMP_PACKBITS):
            for kw in (dict(rows_per_strip=a.shape[1]), dict(rows_per_strip=7), dict(tile=(64, 48)), dict(tile=(128, 128), bigtiff=True),
                       dict(rows_per_strip=1, byteorder=">")):
                for pred in (1, 2):
                    for mode in (R.DEFLATE_MODES if comp == R.COMP_DEFLATE else ("dynamic",)):
                        f, _ = R.write_tiff(a, compression=comp, predictor=pred, deflate_mode=mode, **kw)
                        assert np.array_equal(np.array(Image.open(io.BytesIO(f))), a[0]), (comp, kw, pred, mode)
                        n += 1
    print(f"libtiff {features.version('libtiff')} read {n} files of tests/tiff_reference.py's writer")
    path = os.path.join(HERE, "tiff_libtiff.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", sum(k.endswith("__file") for k in out), "files")


if __name__ == "__main__":
    main()
