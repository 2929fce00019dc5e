"""Reading a window of a scene on the device: read_raster_device(path, window=) against the same slice of the whole device
read, bit for bit, over the layouts of tests/test_tiff_window_host.py with every codec, both predictors and both depths --
the sub-layouts put the kernels of csrc/tiff.hip on a one-strip layout shorter than RowsPerStrip, a one-tile layout smaller
than its tile, and segment offsets of any alignment -- then damaged segments in and outside the window, the host route of an
over-cap Deflate file, an overview level, and the command lines that read windows."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tiff_reference as R  # noqa: E402
from test_tiff_window_host import H, LAYOUTS, W, WINDOWS, _image  # noqa: E402

pytestmark = pytest.mark.gpu


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


@pytest.mark.parametrize("compression", (R.COMP_NONE, R.COMP_LZW, R.COMP_DEFLATE, R.COMP_PACKBITS), ids=lambda c: f"compression{c}")
def test_every_window_equals_the_slice_of_the_whole_device_read(dev, tmp_path, compression):
    """every layout x chunky / planar x predictor 1 / 2, with the band count, the depth, the container and the byte order
    drawn per file (each value is seen); every window of the host matrix, among them the short last strip alone (a one-strip
    sub-layout of 3 rows under RowsPerStrip = 5) and the bottom right edge tile alone (5 x 5 under 16 x 16 and 32 x 16)"""
    import torch
    from lbdrn_hip import raster_io, tiff
    rng = np.random.default_rng(compression)
    seen = set()
    for k, (lay_kw, planar, pred) in enumerate(itertools.product(LAYOUTS, (1, 2), (1, 2))):
        C, bits, big, bo = int(rng.choice([1, 3, 8])), int(rng.choice([8, 16])), bool(rng.integers(2)), str(rng.choice(["<", ">"]))
        seen |= {("C", C), ("bits", bits), ("big", big), ("bo", bo)}
        a = _image(C, np.uint8 if bits == 8 else np.uint16, seed=k)
        path = _write(tmp_path / f"s{k}.tif", R.write_tiff(a, bigtiff=big, byteorder=bo, planar=planar, predictor=pred,
                                                           compression=compression, **lay_kw)[0])
        full = raster_io.read_raster_device(path, dev)
        assert np.array_equal(_host(full), a), (lay_kw, planar, pred)
        for x0, y0, w, h in WINDOWS:
            got = raster_io.read_raster_device(path, dev, window=(x0, y0, w, h))
            assert got.device.type == "cuda" and got.dtype == full.dtype and got.is_contiguous() and tuple(got.shape) == (C, h, w)
            assert torch.equal(got, full[:, y0:y0 + h, x0:x0 + w]), (lay_kw, planar, pred, C, bits, big, bo, (x0, y0, w, h))
        got = raster_io.read_raster(path, window=WINDOWS[5])      # numpy: [h,w] for one band, as the whole read has it
        x0, y0, w, h = WINDOWS[5]
        assert got.dtype == a.dtype and np.array_equal(got, (a[0] if C == 1 else a)[..., y0:y0 + h, x0:x0 + w])
        assert np.array_equal(tiff.read_window(path, WINDOWS[5], dev), a[:, y0:y0 + h, x0:x0 + w])
    assert len(seen) == 9


def test_a_damaged_segment_matters_only_to_the_windows_that_touch_it(dev, tmp_path):
    import torch
    from lbdrn_hip import raster_io, tiff
    a = _image(2)
    kw = dict(tile=(16, 16), compression=R.COMP_DEFLATE, planar=2, predictor=2)
    sound = _write(tmp_path / "sound.tif", R.write_tiff(a, **kw)[0])
    bad = _write(tmp_path / "bad.tif", R.write_tiff(a, segment_hook=lambda i, p: p[:-1] + bytes([p[-1] ^ 1]) if i == 13 else p, **kw)[0])
    with pytest.raises(tiff.TiffError, match=r"segment 13 is damaged: wrong Adler-32"):      # as today
        raster_io.read_raster_device(bad, dev)
    full = raster_io.read_raster_device(sound, dev)
    # segment 13 is band 1's tile at x 16..31, y 0..15
    for x0, y0, w, h in ((0, 0, 16, 16), (32, 0, 5, 53), (0, 16, 37, 37), (3, 20, 30, 9)):
        got = raster_io.read_raster_device(bad, dev, window=(x0, y0, w, h))
        assert torch.equal(got, full[:, y0:y0 + h, x0:x0 + w])
    for window in ((20, 3, 4, 4), (15, 15, 2, 2), (0, 0, W, H)):
        with pytest.raises(tiff.TiffError, match=r"segment 13 is damaged: wrong Adler-32"):      # the file's index, not the plan's
            raster_io.read_raster_device(bad, dev, window=window)


def test_an_over_cap_deflate_strip_file_reads_its_windows_through_the_host_route(dev, tmp_path):
    """strips of 200 rows x 2048 x 16 bit = 800 KiB, above the 768 KiB the device inflates: the whole read and a window of
    a full strip go through zlib on the host, of the touched strips only (strip 0 is damaged and is not inflated); the short
    last strip -- 50 rows, 200 KiB -- is a sub-layout under the cap and is decoded on the device"""
    from lbdrn_hip import raster_io, tiff
    Hh, Ww = 450, 2048
    a = ((np.arange(Hh)[:, None] * 5 + np.arange(Ww)[None, :]) % 60000).astype(np.uint16)[None]
    kw = dict(rows_per_strip=200, planar=1, predictor=2, compression=R.COMP_DEFLATE)
    sound = _write(tmp_path / "sound.tif", R.write_tiff(a, **kw)[0])
    bad = _write(tmp_path / "bad.tif", R.write_tiff(a, segment_hook=lambda i, p: p[:40] if i == 0 else p, **kw)[0])
    scene = tiff.parse(open(sound, "rb").read())
    assert tiff._over_cap(scene.layout, sound) == "host"
    assert tiff._over_cap(tiff.plan_window(scene, (0, 400, 10, 50)).layout, sound) is None
    assert np.array_equal(raster_io.read_raster(sound), a[0])
    for x0, y0, w, h in ((100, 250, 64, 40), (0, 399, Ww, 2), (2000, 420, 48, 30)):
        assert np.array_equal(_host(raster_io.read_raster_device(bad, dev, window=(x0, y0, w, h))), a[:, y0:y0 + h, x0:x0 + w])
        assert np.array_equal(raster_io.read_raster(bad, window=(x0, y0, w, h)), a[0, y0:y0 + h, x0:x0 + w])
    with pytest.raises(tiff.TiffError, match="segment 0 is damaged"):
        raster_io.read_raster(bad, window=(0, 199, 4, 2))


def test_a_window_of_an_overview_level(dev, tmp_path):
    import torch
    from lbdrn_hip import ops, raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(5, 3, 75, 90)
    path = str(tmp_path / "pyramid.tif")
    raster_io.write_raster_device(path, ops.to_device_u16(img, dev), tile=16, overviews="auto")
    for level in (0, 1, 2):
        full = raster_io.read_raster_device(path, dev, overview=level)
        C, Hl, Wl = full.shape
        assert raster_io.raster_shape(path, overview=level) == (C, Hl, Wl, np.dtype(np.uint16))
        for x0, y0, w, h in ((0, 0, 1, 1), (Wl - 1, Hl - 1, 1, 1), (3, 5, Wl - 7, Hl - 9), (14, 15, 4, 3)):
            got = raster_io.read_raster_device(path, dev, overview=level, window=(x0, y0, w, h))
            assert torch.equal(got, full[:, y0:y0 + h, x0:x0 + w]), (level, x0, y0, w, h)
            assert np.array_equal(raster_io.read_raster(path, overview=level, window=(x0, y0, w, h)),
                                  _host(full)[:, y0:y0 + h, x0:x0 + w])
    with pytest.raises(ValueError, match="is not inside"):
        raster_io.read_raster_device(path, dev, overview=1, window=(0, 0, 90, 75))


# ---------------------------------------------------------------- the command lines

def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f if "Time elapsed" not in line]


@pytest.fixture()
def no_launcher(monkeypatch):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBDRN_TILE_READS"):
        monkeypatch.delenv(k, raising=False)


def _whole_then_slice(raster_io):
    """read_raster and read_raster_device in the form they had before they took a window"""
    read, read_device = raster_io.read_raster, raster_io.read_raster_device

    def host(path, overview=0, window=None):
        a = read(path, overview)
        return a if window is None else np.ascontiguousarray(a[..., window[1]:window[1] + window[3], window[0]:window[0] + window[2]])

    def device(path, device="cuda:0", overview=0, window=None):
        t = read_device(path, device, overview)
        return t if window is None else t[:, window[1]:window[1] + window[3], window[0]:window[0] + window[2]]
    return host, device


def test_decode_window_org_and_the_quality_command_line_write_the_records_of_a_whole_read(dev, tmp_path, monkeypatch, no_launcher, capsys):
    import decode
    import encode
    from lbdrn_hip import quality, raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(11, 4, 47, 51)
    src = _write(tmp_path / "scene.tif", R.write_tiff(img, bigtiff=True, tile=(16, 16), planar=2, predictor=2, compression=R.COMP_DEFLATE)[0])
    monkeypatch.setattr(encode, "DEVICE", "cuda:0")
    assert encode.main(["-i", src, "-o", str(tmp_path / "out"), "-K", "4", "-e", "1", "-bs", "256", "-sr", "2"], shard_tiles=False) == 0
    (sub,) = [d for d in (tmp_path / "out").iterdir() if d.is_dir()]
    log, recon = sub / "decode_window.txt", str(tmp_path / "w.tif")
    other = str(tmp_path / "other.npy")
    np.save(other, (img ^ 3)[:, :45, :])
    argv = ["-i", str(sub / "scene.bin"), "--window", "9", "13", "30", "21", "-o", recon, "-org", src, "--metrics"]
    qargv = [src, other, "--window", "9", "13", "30", "21"]
    outside = [src, other, "--window", "9", "13", "30", "33"]

    def run():
        if log.exists():
            os.remove(str(log))
        assert decode.main(argv) == 0
        capsys.readouterr()
        assert quality.main(qargv) == 0
        q = capsys.readouterr()
        assert quality.main(outside) == 2
        return _records(log), q.out, capsys.readouterr().err
    new = run()
    host, device = _whole_then_slice(raster_io)
    monkeypatch.setattr(raster_io, "read_raster", host)
    monkeypatch.setattr(raster_io, "read_raster_device", device)
    old = run()
    assert new == old
    assert sum(r.startswith(("MSE", "PSNR")) for r in new[0]) == 2 and len(new[1].splitlines()) == 5
    assert new[2] == f"--window 9 13 30 33 is not inside {other} (51 x 45)\n"


def test_encode_window_and_tile_reads_write_the_bin_of_the_cropped_file(dev, tmp_path, monkeypatch, no_launcher):
    import encode
    from lbdrn_hip import container
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(7, 4, 96, 128)
    x0, y0, w, h = 13, 9, 101, 75
    stem = f"scene_x{x0}_y{y0}_w{w}_h{h}"
    src = _write(tmp_path / "scene.tif", R.write_tiff(img, tile=(32, 16), planar=2, predictor=2, compression=R.COMP_DEFLATE)[0])
    crop = str(tmp_path / f"{stem}.npy")
    np.save(crop, np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w]))
    monkeypatch.setattr(encode, "DEVICE", "cuda:0")
    flags = ["-sr", "2", "-K", "5", "-D", "2", "-bc", "64", "-nl", "2", "-e", "2", "-bs", "512"]
    win = ["--window"] + [str(v) for v in (x0, y0, w, h)]

    def run(name, path, extra, tile_reads=False):
        monkeypatch.setenv("LBDRN_TILE_READS", "1" if tile_reads else "0")
        assert encode.main(["-i", path, "-o", str(tmp_path / name)] + flags + extra, shard_tiles=False) == 0
        (sub,) = [d for d in (tmp_path / name).iterdir() if d.is_dir()]
        (out,) = [f for f in sub.iterdir() if f.suffix == ".bin"]
        records = [r.replace(str(tmp_path / name), "X") for r in _records(sub / "encode.txt")]
        return out.name, out.read_bytes(), [re.sub(r"fit [0-9.]+s on", "fit on", r) for r in records]
    want = run("crop", crop, [])
    assert container.unpack_header(want[1])[1:4] == (2, w, h)
    got = run("window", src, win)
    assert got[:2] == want[:2] and got[0] == f"{stem}.bin"
    tiles = run("window_tiles", src, win, tile_reads=True)
    assert tiles == got      # the .bin and every record but the times
    whole, whole_tiles = run("whole", src, []), run("whole_tiles", src, [], tile_reads=True)
    assert whole == whole_tiles and whole[0] == "scene.bin" and whole[1] != want[1]
