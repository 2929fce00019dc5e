"""Tiled and compressed TIFF scenes through liblbdrn_tiff.so on the device (csrc/tiff.hip): every layout of the issue on a
base raster of 8 x 37 x 53 uint16 -- 37 and 53 divide by no tile size and no RowsPerStrip used -- the codecs' hard cases,
the files libtiff wrote, the workspace's hygiene on guarded buffers, a fixed list of damaged segments per codec, and the
entry points: raster_io, encode.py and decode.py give from a tiled Deflate predictor-2 BigTIFF what they give from its
uncompressed twin.  Every comparison is exact equality with the source array.

Segment sizes and stream sources here: the largest compressed segment of the base raster is about 31 KB, below Deflate's
32 KiB history ring; the hard cases add a constant raster of 78 KB strips (distance-1 matches only), 7.8 KB of noise and
one 25.6 KB LZW strip; every stream comes from tests/tiff_reference.py (zlib level 9 / Z_FIXED / level 0, the textbook LZW
and PackBits coders) or from libtiff (the golden files).  Segments of a scene's size -- 128 KiB to the caps of 768 KiB, 384 KiB
and 1 MiB of PackBits, zlib levels 1 / 6 / 9, hand-assembled blocks at the ring's edge, codes of 11 to 15 bits, damage beyond
the ring -- are tests/test_gpu_tiff_big.py, on the case table of tests/tiff_big_cases.py.

Every file here except the uncompressed-strip control raised ValueError in raster_io before the library existed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import tiff_reference as R  # noqa: E402
from guarded import FILLS, Arena  # noqa: E402
from test_tiff_host import COMPRESSIONS, base_raster, golden_files, layout_file, layouts  # noqa: E402

pytestmark = pytest.mark.gpu


def device_read(dev, data, tmp_path, name="t.tif"):
    """file bytes -> [C,H,W] numpy through tiff.read_device, which raises on a damaged segment"""
    from lbdrn_hip import tiff
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    t = tiff.read_device(path, dev)
    assert t.is_contiguous() and t.device.type == "cuda" and t.dim() == 3
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


# ---------------------------------------------------------------- layouts

@pytest.mark.parametrize("compression", COMPRESSIONS, ids=lambda c: f"compression{c}")
def test_every_layout_reads_back_exactly(dev, tmp_path, compression):
    """strips of 1, 8 and 37 rows, tiles of 16 x 16 and 32 x 16, chunky and planar, predictor 1 and 2, with the byte order,
    the container, 1 / 3 / 4 / 8 bands and the depth drawn per case (tests/test_tiff_host.py: layouts)"""
    mine = [lay for lay in layouts() if lay["compression"] == compression]
    assert len(mine) == 20
    for lay in mine:
        a, data, info = layout_file(lay)
        got = device_read(dev, data, tmp_path)
        assert got.dtype == a.dtype and np.array_equal(got, a), lay


@pytest.mark.parametrize("compression", COMPRESSIONS, ids=lambda c: f"compression{c}")
def test_296_segments_and_the_band_counts_depths_orders_and_containers(dev, tmp_path, compression):
    """8 planar bands x 37 one-row strips = 296 segments: more than one wave's worth and not a multiple of 64; then every band
    count, depth, byte order and container with this compression"""
    a = base_raster()
    data, info = R.write_tiff(a, rows_per_strip=1, planar=2, predictor=2, compression=compression)
    assert len(info["offsets"]) == 296
    assert np.array_equal(device_read(dev, data, tmp_path), a)
    for bands, dtype, bo, big, seg in ((1, np.uint8, ">", True, dict(tile=(16, 16))), (3, np.uint16, ">", False, dict(rows_per_strip=8)),
                                       (4, np.uint8, "<", False, dict(tile=(32, 16))), (8, np.uint16, ">", True, dict(tile=(32, 16))),
                                       (3, np.uint8, "<", True, dict(rows_per_strip=37)), (1, np.uint16, "<", True, dict(rows_per_strip=8))):
        for planar in (1, 2):
            a = base_raster(dtype=dtype)[:bands]
            data, _ = R.write_tiff(a, byteorder=bo, bigtiff=big, planar=planar, predictor=2, compression=compression, **seg)
            got = device_read(dev, data, tmp_path)
            assert got.dtype == a.dtype and np.array_equal(got, a), (bands, dtype, bo, big, seg, planar)


# ---------------------------------------------------------------- the codecs' hard cases

def test_deflate_block_types_matches_and_literals(dev, tmp_path):
    rng = np.random.default_rng(8)
    const = np.full((2, 37, 530), 40000, np.uint16)      # predictor 2: rows of zeros, distance-1 matches of length 258
    noise = rng.integers(0, 65536, (2, 37, 53)).astype(np.uint16)      # mostly literals
    for a in (const, noise, base_raster()[:3]):
        for mode in R.DEFLATE_MODES:
            for seg in (dict(rows_per_strip=37), dict(tile=(32, 16)), dict(rows_per_strip=8)):
                data, info = R.write_tiff(a, predictor=2, compression=R.COMP_DEFLATE, deflate_mode=mode, planar=1, **seg)
                assert np.array_equal(device_read(dev, data, tmp_path), a), (mode, seg)
    first = R.write_tiff(const, predictor=2, compression=R.COMP_DEFLATE, planar=1)[1]
    assert len(first["raw"][0]) > 100 * len(R.deflate(first["raw"][0]))      # (the constant raster is what it is meant to be)


def test_lzw_clears_widths_and_the_code_that_is_its_own_entry(dev, tmp_path):
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 65536, (1, 64, 200)).astype(np.uint16)      # one strip of 25.6 KB: several Clears, widths 9 to 12
    data, info = R.write_tiff(noise, compression=R.COMP_LZW)
    assert len(info["offsets"]) == 1 and info["counts"][0] * 8 / 12 > 2.5 * 4094
    assert np.array_equal(device_read(dev, data, tmp_path), noise)
    const = np.full((1, 64, 200), 0x2121, np.uint16)      # every code but the first is the entry about to be made
    for pred in (1, 2):
        data, _ = R.write_tiff(const, compression=R.COMP_LZW, predictor=pred)
        assert np.array_equal(device_read(dev, data, tmp_path), const)
    data, _ = R.write_tiff(noise, compression=R.COMP_LZW, predictor=2, rows_per_strip=7, byteorder=">")
    assert np.array_equal(device_read(dev, data, tmp_path), noise)


def test_packbits_runs_of_128_and_the_no_op_byte(dev, tmp_path):
    row = bytes(range(128)) + b"\x05" * 128 + bytes(range(100, 228)) + b"\x09" * 128      # 512 bytes: 256 samples
    a = np.frombuffer(row * 5, "<u2").reshape(1, 5, 256).copy()
    data, info = R.write_tiff(a, compression=R.COMP_PACKBITS, rows_per_strip=1)
    stream = data[info["offsets"][0]:][:info["counts"][0]]
    assert stream[0] == 127 and stream[129] == 0x81 and len(stream) == 2 * 129 + 2 * 2
    assert np.array_equal(device_read(dev, data, tmp_path), a)
    padded, _ = R.write_tiff(a, compression=R.COMP_PACKBITS, rows_per_strip=1,
                             segment_hook=lambda i, p: b"\x80" + p[:129] + b"\x80\x80" + p[129:] + b"\x80")
    assert np.array_equal(device_read(dev, padded, tmp_path), a)


def test_files_libtiff_wrote(dev, tmp_path, golden):
    files = golden_files(golden)
    assert len(files) == 20
    for name, buf, pixels in files:
        if name in ("i16_raw_p1", "i16_raw_p2", "rgb_raw_p1", "rgb_raw_p2"):      # the control: raster_io's own reader
            from lbdrn_hip import raster_io
            path = str(tmp_path / "raw.tif")
            with open(path, "wb") as f:
                f.write(buf)
            assert np.array_equal(raster_io.read_raster(path).reshape(pixels.shape), pixels), name
        got = device_read(dev, buf, tmp_path)
        assert got.dtype == pixels.dtype and np.array_equal(got, pixels), name


# ---------------------------------------------------------------- the C ABI on guarded buffers

def guarded_decode(dev, data, fill, short_by=0):
    """lbdrn_tiff_decode on buffers of tests/guarded.py: (rc, planes [C,H,W], status [nseg], arena, the buffers)"""
    import torch
    from lbdrn_hip import tiff
    sc = tiff.parse(data)
    lay = sc.layout
    L = tiff.lib()
    nseg = len(sc.offsets)
    nws = L.lbdrn_tiff_workspace(ctypes.byref(lay))
    ar = Arena(dev)
    file = ar.const(np.frombuffer(data, np.uint8), name="file")
    planes = ar.buf(lay.C * lay.H * lay.W * (lay.bits // 8), fill, name="planes")
    status = ar.buf(4 * nseg, fill, name="status")
    ws = ar.buf(nws - short_by, fill, name="workspace")
    offsets, counts = np.ascontiguousarray(sc.offsets), np.ascontiguousarray(sc.counts)
    rc = L.lbdrn_tiff_decode(ctypes.byref(lay), file.ptr, len(data), offsets.ctypes.data, counts.ctypes.data, nseg, planes.ptr,
                             status.ptr, ws.ptr, nws - short_by, None)
    torch.cuda.synchronize(dev)
    out = planes.numpy(np.uint8 if lay.bits == 8 else np.uint16).reshape(lay.C, lay.H, lay.W)
    return rc, out, status.numpy(np.int32), ar, (planes, status, ws)


@pytest.mark.parametrize("compression", COMPRESSIONS, ids=lambda c: f"compression{c}")
def test_workspace_hygiene(dev, compression):
    """fills 0x00 / 0xFF / 0xA5 of workspace, planes and status give the same bits; the guards and the file are intact; status is
    all zero; a workspace one byte short is refused before a launch"""
    from lbdrn_hip import tiff
    a = base_raster()[:4]
    for seg in (dict(tile=(16, 16), planar=1), dict(rows_per_strip=8, planar=2)):
        data, _ = R.write_tiff(a, predictor=2, compression=compression, byteorder=">", **seg)
        for fill in FILLS:
            rc, out, status, ar, _ = guarded_decode(dev, data, fill)
            assert rc == 0, (tiff.lib().lbdrn_tiff_last_error(), fill)
            ar.check()
            assert not status.any() and np.array_equal(out, a), (seg, fill)
        rc, out, status, ar, (planes, st, ws) = guarded_decode(dev, data, 0xA5, short_by=1)
        assert rc == tiff.E_WORKSPACE and b"workspace" in tiff.lib().lbdrn_tiff_last_error()
        ar.check()
        for b in (planes, st, ws):      # nothing was launched: every buffer still holds its fill
            assert bool((b.as_u8() == 0xA5).all()), b.name


@pytest.mark.parametrize("compression", (R.COMP_DEFLATE, R.COMP_LZW, R.COMP_PACKBITS), ids=lambda c: f"compression{c}")
def test_damaged_segments_are_flagged_and_touch_nothing_else(dev, compression):
    """the fixed list of tests/tiff_reference.py (the sanitized host program of tests/test_tiff_host.py runs the same cases on the
    same csrc/tiff.inc): segment 1 of five strips damaged.  Its status is non-zero, every other strip is exact, the guards
    are intact."""
    a = base_raster()[:1]
    sound, info = R.write_tiff(a, rows_per_strip=8, predictor=2, compression=compression)
    k = 1
    stream = sound[info["offsets"][k]:][:info["counts"][k]]
    cases = R.damage_cases(compression, stream, len(info["raw"][k]))
    assert 19 <= len(cases) <= 22
    for name, bad in cases:
        data, _ = R.write_tiff(a, rows_per_strip=8, predictor=2, compression=compression, segment_hook=lambda i, p: bad if i == k else p)
        rc, out, status, ar, _ = guarded_decode(dev, data, 0xA5)
        assert rc == 0, name
        ar.check()
        assert status[k] != 0 and not np.delete(status, k).any(), (name, status)
        keep = np.ones(37, bool)
        keep[8 * k:8 * k + 8] = False
        assert np.array_equal(out[:, keep], a[:, keep]), name
    # an uncompressed strip shorter than its rows: status 1, the other strips exact
    data, info = R.write_tiff(a, rows_per_strip=8, segment_hook=lambda i, p: p[:-1] if i == k else p)
    rc, out, status, ar, _ = guarded_decode(dev, data, 0xFF)
    ar.check()
    assert rc == 0 and status.tolist() == [0, 1, 0, 0, 0] and np.array_equal(out[:, 16:], a[:, 16:]) and np.array_equal(out[:, :8], a[:, :8])


def test_read_device_raises_with_the_damaged_segments_index(dev, tmp_path):
    from lbdrn_hip import tiff
    a = base_raster()[:2]
    data, _ = R.write_tiff(a, tile=(16, 16), compression=R.COMP_DEFLATE, planar=2,
                           segment_hook=lambda i, p: p[:-1] + bytes([p[-1] ^ 1]) if i == 13 else p)
    with pytest.raises(tiff.TiffError, match=r"segment 13 is damaged: wrong Adler-32"):
        device_read(dev, data, tmp_path)


# ---------------------------------------------------------------- entry points and the command line

@pytest.fixture(scope="module")
def twins(tmp_path_factory, dev):
    """the 4 x 47 x 51 scene of tests/test_gpu_sweep_in_flight.py, as raster_io writes it and as a tiled Deflate predictor-2
    BigTIFF: two files named scene.tif"""
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(11, 4, 47, 51)
    root = tmp_path_factory.mktemp("twins")
    (root / "plain").mkdir()
    (root / "packed").mkdir()
    plain, packed = str(root / "plain" / "scene.tif"), str(root / "packed" / "scene.tif")
    raster_io.write_raster(plain, img)
    with open(packed, "wb") as f:
        f.write(R.write_tiff(img, bigtiff=True, tile=(16, 16), planar=2, predictor=2, compression=R.COMP_DEFLATE)[0])
    return img, plain, packed, root


def test_read_raster_and_read_raster_device(dev, twins):
    import torch
    from lbdrn_hip import raster_io
    img, plain, packed, _ = twins
    for path in (plain, packed):
        a = raster_io.read_raster(path)
        assert a.dtype == np.uint16 and a.shape == (4, 47, 51) and np.array_equal(a, img)
        t = raster_io.read_raster_device(path, dev)
        assert t.device.type == "cuda" and t.dtype == torch.int16 and t.is_contiguous() and tuple(t.shape) == (4, 47, 51)
        assert np.array_equal(t.cpu().numpy().view(np.uint16), img)
    assert raster_io.raster_size(packed) == (51, 47)


def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f]


def test_cli_writes_the_same_bitstream_and_records_from_both_twins(dev, twins, monkeypatch):
    import decode
    import encode
    img, plain, packed, root = twins
    monkeypatch.setattr(encode, "DEVICE", "cuda:0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bins = []
    for name, src in (("plain", plain), ("packed", packed)):
        out = root / f"out_{name}"
        assert encode.main(["-i", src, "-o", str(out), "-K", "4", "-e", "2", "-bs", "256", "-sr", "2"], shard_tiles=False) == 0
        (sub,) = [d for d in out.iterdir() if d.is_dir()]
        bins.append(sub / "scene.bin")
    assert bins[0].read_bytes() == bins[1].read_bytes()
    logs = []
    for src in (plain, packed):      # decode.py -org: the same stream measured against each twin
        log = bins[0].parent / "decode.txt"
        if log.exists():
            os.remove(str(log))
        assert decode.main(["-i", str(bins[0]), "-org", src]) == 0
        logs.append([r for r in _records(log) if r.startswith(("MSE", "PSNR"))])
    assert logs[0] == logs[1] and len(logs[0]) >= 2 and any(r.startswith("MSE") for r in logs[0])
