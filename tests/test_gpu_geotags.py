"""encode.py --keep-tags / decode.py on the GPU: the tags of a georeferenced scene come back on the decoded raster -- as stored
for a whole decode, moved to the window's origin for --window --, on every writer path (today's writer, --out-compress with and
without overviews, the merged tiles of -sr 2, the pieces of a window), and nothing else about the raster changes.

A 4 x 32 x 36 scene (the size of tests/test_gpu_window_decode.py's command-line cases), one epoch; encoded once per module at
-sr 1, at -sr 2 and at -sr 2 with --max-error 0.  At -sr 2 the tiles are 18 x 16: the window (10, 9, 17, 13) crosses both seams."""
import os
import shutil
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tiff_reference as TR  # noqa: E402
from pyramid_helpers import GEO, with_tags  # noqa: E402
from test_gpu_window_decode import _records, _settings  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE = (4, 32, 36)
TAGS = [GEO[0], GEO[1]] + GEO[3:]      # pixel scale, one tiepoint, the GeoKey tags, GDAL_METADATA, GDAL_NODATA "0"
OTHER = [(33550, 12, 3, struct.pack("<3d", 0.5, 0.5, 0.0)), (33922, 12, 6, struct.pack("<6d", 0, 0, 0, 1.0, 2.0, 0)), (42113, 2, 4, b"255\0")]
WINDOW = (10, 9, 17, 13)
ENCODE = {"one": ["-sr", "1"], "two": ["-sr", "2"], "lossless": ["-sr", "2", "--max-error", "0"]}
_BUILT = {}


class Case:
    pass


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("geotags")


def _tiff(path, img, tags):
    data = TR.write_tiff(img, rows_per_strip=8)[0]
    with open(path, "wb") as f:
        f.write(with_tags(data, tags) if tags else data)
    return str(path)


def case(name, work):
    """the scene encoded with --keep-tags, and the same .bin without its chunk in a directory of its own; once per module"""
    if name in _BUILT:
        return _BUILT[name]
    import encode
    from lbdrn_hip import container
    from lbdrn_hip.synth import synthetic_tile
    c = Case()
    c.img = synthetic_tile(41, *SHAPE).astype(np.uint16)
    c.img[:, 5:8, 9:14] = 0      # nodata samples that share 2 x 2 blocks with data
    c.src = _tiff(work / "scene.tif", c.img, TAGS)
    with _settings():
        assert encode.main(["-i", c.src, "-o", str(work / name), "-e", "1", "-bs", "512", "-D", "2", "--keep-tags"] + ENCODE[name]) == 0
    (sub,) = [p for p in (work / name).iterdir() if p.is_dir()]
    c.dir, c.bin = sub, str(sub / "scene.bin")
    c.raw = open(c.bin, "rb").read()
    assert container.unpack_geo_trailer(c.raw) == TAGS and c.raw.endswith(container.pack_geo_trailer(TAGS))
    assert _records(sub / "encode.txt")[-2] == f"Tags: {len(TAGS)} tags, {len(container.pack_geo_trailer(TAGS))} bytes"
    c.bare_dir = work / (name + "-bare")
    c.bare_dir.mkdir()
    c.bare = str(c.bare_dir / "scene.bin")
    with open(c.bare, "wb") as f:
        f.write(container.strip_geo_trailer(c.raw))
    assert (container.unpack_residual_trailer(c.raw) is not None) == (name == "lossless")
    assert container.unpack_residual_trailer(c.raw) == container.unpack_residual_trailer(open(c.bare, "rb").read())
    _BUILT[name] = c
    return c


def decode_to(bin_path, keep, flags=()):
    """decode.main on bin_path -> (the raster's bytes, its path kept under `keep`, the records of this run)"""
    import decode
    d = os.path.dirname(bin_path)
    for log in ("decode.txt", "decode_window.txt"):
        if os.path.exists(os.path.join(d, log)):
            os.remove(os.path.join(d, log))
    with _settings():
        assert decode.main(["-i", bin_path] + list(flags)) == 0
    out = flags[flags.index("-o") + 1] if "-o" in flags else os.path.join(d, "scene_recon.tif")
    shutil.copyfile(out, keep)
    log = "decode_window.txt" if "--window" in flags else "decode.txt"
    return open(keep, "rb").read(), str(keep), _records(os.path.join(d, log))


def ifd_tags(data):
    """the tag numbers of every IFD of a classic little-endian TIFF, in chain order"""
    assert data[:4] == b"II*\0"
    out, off = [], struct.unpack_from("<I", data, 4)[0]
    while off:
        n = struct.unpack_from("<H", data, off)[0]
        out.append([struct.unpack_from("<H", data, off + 2 + 12 * i)[0] for i in range(n)])
        off = struct.unpack_from("<I", data, off + 2 + 12 * n)[0]
    return out


@pytest.mark.parametrize("name", ("one", "two"))
def test_round_trip_restores_the_tags_and_no_tags_ignores_them(name, dev, work):
    from lbdrn_hip import raster_io
    c = case(name, work)
    kept, kept_path, recs = decode_to(c.bin, work / f"{name}-kept.tif")
    bare, bare_path, recs_bare = decode_to(c.bare, work / f"{name}-bare.tif")
    assert raster_io.read_geo_tags(kept_path) == TAGS == raster_io.read_geo_tags(c.src)
    assert raster_io.read_geo_tags(bare_path) == []
    a, b = raster_io.read_raster(kept_path), raster_io.read_raster(bare_path)
    assert a.shape == SHAPE and a.dtype == np.uint16 and np.array_equal(a, b)
    assert f"Tags: {len(TAGS)} tags restored" in recs and not any(r.startswith("Tags") for r in recs_bare)
    assert [r for r in recs if not r.startswith(("Tags", "Time elapsed"))] == \
        [r.replace(str(c.bare_dir), str(c.dir)) for r in recs_bare if not r.startswith("Time elapsed")]
    # --no-tags: byte for byte the raster of the file without the chunk, and its records
    ignored, _, recs_ignored = decode_to(c.bin, work / f"{name}-ignored.tif", ["--no-tags"])
    assert ignored == bare and not any(r.startswith("Tags") for r in recs_ignored)


@pytest.mark.parametrize("name", ("one", "two"))
def test_with_pyramids_the_tags_ride_the_first_ifd_and_the_nodata_is_the_stored_one(name, dev, work):
    """-sr 1: the reconstruction is compressed where it lies; -sr 2: the merged tiles are uploaded once.  Either way the file is
    the one --out-nodata 0 --out-georef SCENE writes."""
    from lbdrn_hip import geotags, raster_io
    c = case(name, work)
    flags = ["--out-compress", "deflate", "--out-tile", "16", "--out-overviews", "auto"]
    got, path, recs = decode_to(c.bin, work / f"{name}-pyr.tif", flags)
    levels = ifd_tags(got)
    assert len(levels) >= 2 and all(t in levels[0] for t, _, _, _ in TAGS)
    assert not any(t in geotags.NAMES for lv in levels[1:] for t in lv)
    assert raster_io.read_geo_tags(path) == TAGS and geotags.stored_nodata(TAGS, 16) == 0
    explicit = flags + ["--out-nodata", "0", "--out-georef", c.src]
    assert got == decode_to(c.bare, work / f"{name}-pyr-explicit.tif", explicit)[0]
    assert got == decode_to(c.bin, work / f"{name}-pyr-explicit2.tif", explicit)[0]
    assert f"Tags: {len(TAGS)} tags restored" in recs
    # the file without the chunk: today's pyramid, no tag on any IFD, the same full resolution
    plain, plain_path, _ = decode_to(c.bare, work / f"{name}-pyr-plain.tif", flags)
    assert len(ifd_tags(plain)) == len(levels) and not any(t in geotags.NAMES for lv in ifd_tags(plain) for t in lv)
    assert np.array_equal(raster_io.read_raster(path), raster_io.read_raster(plain_path))


def test_a_window_across_the_seam_carries_the_tags_of_the_crop(dev, work):
    from lbdrn_hip import geotags, raster_io
    c = case("two", work)
    x0, y0, w, h = WINDOW
    whole = raster_io.read_raster(decode_to(c.bare, work / "two-whole.tif")[1])
    moved = geotags.shift(TAGS, x0, y0)
    assert struct.unpack("<6d", moved[1][3]) == (0.0, 0.0, 0.0, 399960.0 + 10 * x0, 5700000.5 - 10 * y0, 0.0)
    win = ["--window"] + [str(v) for v in WINDOW]
    for tag, extra in (("plain", []), ("deflate", ["--out-compress", "deflate", "--out-tile", "16"])):
        out = str(work / f"window-{tag}-out.tif")
        _, path, recs = decode_to(c.bin, work / f"window-{tag}.tif", win + ["-o", out] + extra)
        assert raster_io.read_geo_tags(path) == moved != TAGS
        assert np.array_equal(raster_io.read_raster(path), whole[:, y0:y0 + h, x0:x0 + w])
        assert f"Tags: {len(TAGS)} tags restored" in recs
        ignored = decode_to(c.bin, work / f"window-{tag}-ignored.tif", win + ["-o", out, "--no-tags"] + extra)[0]
        assert ignored == decode_to(c.bare, work / f"window-{tag}-bare.tif", win + ["-o", out] + extra)[0]
    # a window at the origin: the tags as stored
    _, path, _ = decode_to(c.bin, work / "window-origin.tif", ["--window", "0", "0", "20", "11", "-o", str(work / "window-origin-out.tif")])
    assert raster_io.read_geo_tags(path) == TAGS


def test_lossless_with_tags_gives_the_original_raster_and_its_tags(dev, work):
    from lbdrn_hip import raster_io
    c = case("lossless", work)
    _, path, recs = decode_to(c.bin, work / "lossless.tif")
    assert np.array_equal(raster_io.read_raster(path), c.img) and raster_io.read_geo_tags(path) == TAGS
    assert "Residual layer: max error 0" in recs and f"Tags: {len(TAGS)} tags restored" in recs
    x0, y0, w, h = WINDOW
    _, path, _ = decode_to(c.bin, work / "lossless-window.tif", ["--window"] + [str(v) for v in WINDOW] + ["-o", str(work / "lossless-window-out.tif")])
    assert np.array_equal(raster_io.read_raster(path), c.img[:, y0:y0 + h, x0:x0 + w])
    # the stored nodata is used, not only written: with the scene's zeros back in place, the overviews are those of --out-nodata 0
    # and not those of a run that names no nodata
    flags = ["--out-compress", "deflate", "--out-tile", "16", "--out-overviews", "auto"]
    got, path, _ = decode_to(c.bin, work / "lossless-pyr.tif", flags)
    assert got == decode_to(c.bare, work / "lossless-pyr-explicit.tif", flags + ["--out-nodata", "0", "--out-georef", c.src])[0]
    _, unaware, _ = decode_to(c.bare, work / "lossless-pyr-unaware.tif", flags + ["--out-georef", c.src])
    assert np.array_equal(raster_io.read_raster(path), raster_io.read_raster(unaware))
    assert not np.array_equal(raster_io.read_raster(path, overview=1), raster_io.read_raster(unaware, overview=1))


def test_out_georef_wins_over_the_stored_tags(dev, work):
    from lbdrn_hip import raster_io
    c = case("one", work)
    other = _tiff(work / "other.tif", c.img, OTHER)
    flags = ["--out-compress", "deflate", "--out-tile", "16", "--out-georef", other]
    got, path, recs = decode_to(c.bin, work / "georef.tif", flags)
    assert raster_io.read_geo_tags(path) == OTHER and not any(r.startswith("Tags") for r in recs)
    assert got == decode_to(c.bare, work / "georef-bare.tif", flags)[0]


def test_a_npy_output_from_a_tagged_file(dev, work):
    c = case("two", work)
    x0, y0, w, h = WINDOW
    out = str(work / "window.npy")
    _, path, recs = decode_to(c.bin, work / "window-copy.npy", ["--window"] + [str(v) for v in WINDOW] + ["-o", out])
    bare = decode_to(c.bare, work / "window-bare.npy", ["--window"] + [str(v) for v in WINDOW] + ["-o", out])[1]
    assert np.array_equal(np.load(path), np.load(bare)) and np.load(path).shape == (4, h, w)
    assert not any(r.startswith("Tags") for r in recs)
