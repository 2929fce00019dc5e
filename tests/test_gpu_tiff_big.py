"""liblbdrn_tiff.so on segments of a scene's size (csrc/tiff.hip, csrc/tiff.inc with 64 lanes): the case table of
tests/tiff_big_cases.py, which tests/test_tiff_host_big.py runs through the one-lane host build, on the device.

  - every row as a strip of a one-band 8-bit raster, rows of one size as the strips of one raster (a launch of several
    waves), on guarded buffers under two fills: rc 0, every status 0, the planes equal to the row's expected bytes;
  - whole files at tile size through tiff.read_device against the source array: 4- and 8-band uint16 and 3-band uint8 rasters
    of 270 x 300 (edge tiles 44 wide and 14 high), tiles of 256 x 256 planar, 128 x 128 chunky and 512 x 16 (wider than the
    raster), strips of 64 and 300 rows, Deflate at zlib level 9 with both predictors and byte orders, LZW on a covering set;
    the 8-band chunky 256 x 256 tile (1 MiB) takes the host route with Deflate and the named refusal with LZW;
  - the package's own writer to its reader with one strip of exactly the Deflate cap;
  - damaged segments longer than the history ring between two sound ones: flagged, the neighbours exact, the guards intact.

Every comparison is exact equality."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tiff_big_cases as B  # noqa: E402
import tiff_reference as R  # noqa: E402
from test_gpu_tiff import device_read, guarded_decode  # noqa: E402

pytestmark = pytest.mark.gpu


def shape_of(n):
    """(H, W) of a one-band 8-bit strip of n bytes: the widest row of at most 2048 samples that divides it"""
    W = max(w for w in range(1, 2049) if n % w == 0)
    return n // W, W


def strips_file(codec, streams, n):
    """a one-band 8-bit raster whose strips are these streams, each of n bytes once decoded"""
    H, W = shape_of(n)
    a = np.zeros((1, H * len(streams), W), np.uint8)
    data, info = R.write_tiff(a, rows_per_strip=H, compression=codec, packed=list(streams), raw=[b""] * len(streams))
    assert len(info["offsets"]) == len(streams)
    return data


# ---------------------------------------------------------------- every row of the table

GROUPS = {"deflate-zlib": (R.COMP_DEFLATE, ("zlib-", "adler-")), "deflate-hand": (R.COMP_DEFLATE, ("hand-", "stop-")),
          "lzw": (R.COMP_LZW, ("lzw-",)), "packbits": (R.COMP_PACKBITS, ("packbits-",))}


def test_the_groups_cover_the_table():
    mine = [r[0] for codec, prefixes in GROUPS.values() for r in B.rows() if r[1] == codec and r[0].startswith(prefixes)]
    assert sorted(mine) == sorted(r[0] for r in B.rows())


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_every_row_of_the_table_on_the_device(dev, group):
    from lbdrn_hip import tiff
    assert tiff.lib().lbdrn_tiff_segment_cap(R.COMP_DEFLATE) == B.CAP_DEFLATE and tiff.lib().lbdrn_tiff_segment_cap(R.COMP_LZW) == B.CAP_LZW
    codec, prefixes = GROUPS[group]
    by_size = {}
    for row in B.rows():
        if row[1] == codec and row[0].startswith(prefixes):
            by_size.setdefault(len(row[3]), []).append(row)
    assert by_size
    for n, rows in by_size.items():
        names = [r[0] for r in rows]
        data = strips_file(codec, [r[2] for r in rows], n)
        want = b"".join(r[3] for r in rows)
        seen = []
        for fill in (0x00, 0xA5):
            rc, out, status, ar, _ = guarded_decode(dev, data, fill)
            assert rc == 0, (tiff.lib().lbdrn_tiff_last_error(), names)
            ar.check()
            assert not status.any(), (names, status)
            got = out.tobytes()
            if got != want:
                k = int(np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0])
                raise AssertionError(f"{names[k // n]}: the first wrong byte is byte {k % n} of {n} (fill {fill:#x})")
            seen.append(got)
        assert seen[0] == seen[1]


# ---------------------------------------------------------------- whole files at tile size

LAYOUTS = (dict(tile=(256, 256), planar=2), dict(tile=(128, 128), planar=1), dict(tile=(512, 16), planar=1),
           dict(rows_per_strip=64, planar=1), dict(rows_per_strip=300, planar=2))
CODINGS = ((1, "<"), (2, ">"), (2, "<"), (1, ">"))      # (predictor, byte order)
RASTERS = {"u16x4": (4, np.uint16), "u16x8": (8, np.uint16), "u8x3": (3, np.uint8)}


def tile_raster(name):
    C, dtype = RASTERS[name]
    a = B.base_raster_like(C, 270, 300, 40 + C)
    return a if dtype == np.uint16 else (a >> 3).astype(np.uint8)


@pytest.mark.parametrize("raster", sorted(RASTERS))
def test_whole_files_at_tile_size_deflate(dev, tmp_path, raster):
    """every layout x predictor x byte order, zlib level 9"""
    a = tile_raster(raster)
    for lay in LAYOUTS:
        for pred, bo in CODINGS:
            data, info = R.write_tiff(a, compression=R.COMP_DEFLATE, predictor=pred, byteorder=bo, **lay)
            assert max(len(r) for r in info["raw"]) <= B.CAP_DEFLATE
            got = device_read(dev, data, tmp_path)
            assert got.dtype == a.dtype and np.array_equal(got, a), (lay, pred, bo)


@pytest.mark.parametrize("raster", sorted(RASTERS))
def test_whole_files_at_tile_size_lzw(dev, tmp_path, raster):
    """one (predictor, byte order) per layout and raster, drawn so that over the three rasters every layout meets both
    predictors and both byte orders (the Python LZW coder is what takes the time); the 8-band raster on its chunky layouts"""
    a = tile_raster(raster)
    r = sorted(RASTERS).index(raster)
    n = 0
    for i, lay in enumerate(LAYOUTS):
        if raster == "u16x8" and lay["planar"] == 2:
            continue
        pred, bo = CODINGS[(i + r) % 4]
        data, info = R.write_tiff(a, compression=R.COMP_LZW, predictor=pred, byteorder=bo, **lay)
        assert max(len(s) for s in info["raw"]) <= B.CAP_LZW
        got = device_read(dev, data, tmp_path)
        assert got.dtype == a.dtype and np.array_equal(got, a), (lay, pred, bo)
        n += 1
    assert n == (3 if raster == "u16x8" else 5)


def test_the_one_mebibyte_chunky_tile_is_above_the_caps(dev, tmp_path):
    """8 bands x 256 x 256 x 16 bit in one chunky tile: Deflate is inflated on the host and placed in numpy, LZW is refused by
    name before any device work"""
    from lbdrn_hip import tiff
    a = tile_raster("u16x8")
    data, info = R.write_tiff(a, tile=(256, 256), planar=1, predictor=2, compression=R.COMP_DEFLATE, byteorder=">")
    assert len(info["raw"][0]) == 1 << 20 > B.CAP_DEFLATE
    assert tiff._over_cap(tiff.parse(data).layout, "scene.tif") == "host"
    assert np.array_equal(device_read(dev, data, tmp_path), a)
    fake, _ = R.write_tiff(a, tile=(256, 256), planar=1, predictor=2, compression=R.COMP_LZW, packed=[R.lzw_encode(b"")] * 4)
    with pytest.raises(ValueError, match=rf"a segment of {1 << 20} bytes is above the cap of {B.CAP_LZW} bytes"):
        device_read(dev, fake, tmp_path)


# ---------------------------------------------------------------- the package's writer to its reader, at the cap

@pytest.mark.parametrize("content", ("smooth", "noise32768"))
def test_writer_to_reader_with_one_strip_of_exactly_the_cap(dev, tmp_path, content):
    import torch
    from lbdrn_hip import tiff, tiff_write
    if content == "smooth":
        a, pred = B.base_raster_like(1, 384, 1024, 51), 2
    else:
        a, pred = np.frombuffer(B.periodic_noise(B.RING, B.CAP_DEFLATE, 52), "<u2").reshape(1, 384, 1024).copy(), 1
    assert a.nbytes == B.CAP_DEFLATE
    path = str(tmp_path / "cap.tif")
    tiff_write.write_device(path, torch.from_numpy(a.view(np.int16)).to(dev), "deflate", rows_per_strip=384, predictor=pred)
    buf = open(path, "rb").read()
    sc = tiff.parse(buf)
    assert len(sc.offsets) == 1 and tiff._segment_bytes(sc.layout) == B.CAP_DEFLATE and sc.layout.predictor == pred
    (raw,) = R.raw_segments(a, rows_per_strip=384, predictor=pred)
    assert zlib.decompress(buf[int(sc.offsets[0]):][:int(sc.counts[0])]) == raw      # zlib reads the writer's stream
    assert np.array_equal(device_read(dev, buf, tmp_path, "again.tif"), a)


# ---------------------------------------------------------------- damage at size

@pytest.mark.parametrize("compression", (R.COMP_DEFLATE, R.COMP_LZW), ids=lambda c: f"compression{c}")
def test_damaged_large_segments_are_flagged_and_touch_nothing_else(dev, compression):
    """tests/tiff_big_cases.py: damage_rows, each between two sound strips of its size.  The damaged strip's status is the one
    the row names (any non-zero one where it names none), the sound strips are exact, the guards are intact."""
    rows = [r for r in B.damage_rows() if r[1] == compression]
    assert len(rows) == (5 if compression == R.COMP_DEFLATE else 2)
    for name, codec, bad, want, sound, expected in rows:
        n = len(expected)
        assert n > B.RING
        data = strips_file(codec, [sound, bad, sound], n)
        rc, out, status, ar, _ = guarded_decode(dev, data, 0xA5)
        assert rc == 0, name
        ar.check()
        assert status[0] == 0 and status[2] == 0 and status[1] != 0 and (want is None or status[1] == want), (name, status)
        H = out.shape[1] // 3
        assert out[:, :H].tobytes() == expected and out[:, 2 * H:].tobytes() == expected, name
