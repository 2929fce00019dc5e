"""The overview pyramid through liblbdrn_pyramid.so on the device (csrc/pyramid.hip): every level against
tests/pyramid_reference.py on the shapes, options and data classes of tests/pyramid_helpers.py; the vector and the scalar path
(widths that hit and miss the vector width, views with an odd element offset and an odd row pitch, views that keep the
alignment); the C ABI on guarded buffers under three fills, on two runs and on a second stream; pyramidal files written by
raster_io.write_raster_device and read back level by level; decode.py --out-overviews / --out-georef; and the converter,
python -m lbdrn_hip.pyramid.  Every comparison is exact: the reduction is integer arithmetic.

Nothing here ran before the library existed: lbdrn_hip.pyramid, liblbdrn_pyramid.so and the options are new."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyramid_helpers as H  # noqa: E402
import tiff_write_helpers as TW  # noqa: E402
from guarded import FILLS, Arena  # noqa: E402

pytestmark = pytest.mark.gpu
R = H.R


def to_device(a, dev):
    import torch
    a = np.array(a, order="C")      # (a writable copy: torch wants one)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def to_host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def assert_levels(got, want, label):
    assert len(got) == len(want), label
    for k, (g, w) in enumerate(zip(got, want), 1):
        g = to_host(g)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (label, k)


# ---------------------------------------------------------------- against the reference

@pytest.mark.parametrize("shape", H.SHAPES, ids=H.shape_id)
def test_device_equals_reference_on_every_level(dev, shape):
    from lbdrn_hip import pyramid
    n = 0
    for dtype, resampling, nodata, data, a, want in H.cases(shape):
        got = pyramid.build(to_device(a, dev), len(want), resampling, nodata)
        assert_levels(got, want, (shape, np.dtype(dtype).name, resampling, nodata, data))
        assert got[-1].shape == (shape[0], 1, 1) and all(g.is_contiguous() for g in got)
        n += 1
    assert n == 36
    if shape == (1, 3, 3):
        assert np.array_equal(to_host(pyramid.build(to_device(H.EXAMPLE, dev), 1)[0]), H.EXAMPLE_LEVEL)


@pytest.mark.parametrize("dtype", (np.uint16, np.uint8), ids=("u16", "u8"))
def test_vector_and_scalar_paths(dev, dtype):
    """W = 129, 130, 136: rows whose tail is 1, 2 and 0 samples of a vector; contiguous rasters (rows of an odd width start off
    16 bytes every other row), views with an odd element offset and an odd row pitch (no lane finds its alignment: the scalar
    path alone), views that start on 32 samples with a pitch of 160 (the vector path in a view)"""
    from lbdrn_hip import pyramid
    top = H.top_of(dtype)
    Hh, C = 11, 2
    for W in (129, 130, 136):
        odd_w = (W + 7) | 1
        odd = H.raster((C, Hh + 3, odd_w), dtype, "random", None, seed=W)
        even = H.raster((C, Hh + 2, 192), dtype, "random", None, seed=W + 1)
        t_odd, t_even = to_device(odd, dev), to_device(even, dev)
        views = (("contiguous", to_device(odd[:, :Hh, :W], dev), odd[:, :Hh, :W]),
                 ("odd offset, odd pitch", t_odd[:, 1:1 + Hh, 3:3 + W], odd[:, 1:1 + Hh, 3:3 + W]),
                 ("aligned view", t_even[:, 2:2 + Hh, 32:32 + W], even[:, 2:2 + Hh, 32:32 + W]))
        for name, t, a in views:
            assert name == "contiguous" or not t.is_contiguous()
            if name == "odd offset, odd pitch":
                assert t.stride(1) % 2 == 1 and (t.storage_offset() % 2 == 1 or t.stride(1) % 2 == 1)
            for resampling in H.RESAMPLINGS:
                for nodata in (None, 0, top):
                    want = R.pyramid(np.ascontiguousarray(a), 3, resampling, nodata)
                    assert_levels(pyramid.build(t, 3, resampling, nodata), want, (W, name, resampling, nodata))
    # many workgroups, every plane: a raster of some hundred thousand vectors
    big = H.raster((3, 515, 2050), dtype, "random", None, seed=9)
    for resampling, nodata in (("average", None), ("average", top), ("nearest", None)):
        assert_levels(pyramid.build(to_device(big, dev), 4, resampling, nodata), R.pyramid(big, 4, resampling, nodata), ("big", resampling, nodata))


# ---------------------------------------------------------------- the C ABI on guarded buffers

def guarded_build(dev, a, levels, fill, resampling=0, nodata=None, stream=None, short_by=0):
    """lbdrn_pyr_build on buffers of tests/guarded.py: (rc, the output's bytes, arena, output buffer)"""
    import torch
    from lbdrn_hip import pyramid
    L = pyramid.lib()
    C, Hh, W = a.shape
    d = pyramid.Desc(C, Hh, W, a.dtype.itemsize * 8, resampling, nodata is not None, nodata or 0, 0, W, Hh * W)
    need = L.lbdrn_pyr_output_bytes(ctypes.byref(d), levels)
    ar = Arena(dev)
    src = ar.const(a, name="src")
    out = ar.buf(need - short_by, fill, name="out")
    rc = L.lbdrn_pyr_build(ctypes.byref(d), src.ptr, levels, out.ptr, need - short_by, None if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, out.numpy(np.uint8), ar, out


def test_output_hygiene_determinism_and_a_second_stream(dev, tmp_path_factory):
    """fills 0x00 / 0xFF / 0xA5 of the output give the same levels and leave the padding between them as it was; the guards
    and the source are intact; two runs and a run on another stream give the same bits; an output one byte short is refused
    before a launch"""
    import torch
    from lbdrn_hip import pyramid
    shim = H.load_shim(tmp_path_factory)
    for shape, dtype, resampling, nodata in (((8, 75, 130), np.uint16, "average", 0), ((2, 37, 53), np.uint8, "average", None),
                                             ((3, 5, 130), np.uint16, "nearest", None), ((1, 65, 129), np.uint8, "average", 255)):
        a = H.raster(shape, dtype, "random", nodata)
        levels = R.max_levels(*shape[1:])
        want = R.pyramid(a, levels, resampling, nodata)
        first = None
        for fill in FILLS + (0xA5,):      # (0xA5 twice: two runs)
            rc, raw, ar, _ = guarded_build(dev, a, levels, fill, H.R_CODE[resampling], nodata)
            assert rc == 0, (pyramid.lib().lbdrn_pyr_last_error(), fill)
            ar.check()
            got = H.split_levels(shim, raw, *shape, levels, dtype)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), (shape, fill)
            used = np.zeros(raw.size, bool)
            for k, lv in enumerate(got, 1):
                at = shim.pyr_shim_level_offset(*shape, k, a.dtype.itemsize)
                used[at:at + lv.nbytes] = True
            assert (~used).any() and (raw[~used] == fill).all(), "the padding between two levels was written"
            if fill == 0xA5:
                first = raw if first is None else first
                assert np.array_equal(raw, first)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            rc, raw, ar, _ = guarded_build(dev, a, levels, 0xA5, H.R_CODE[resampling], nodata, stream=side)
        ar.check()
        assert rc == 0 and np.array_equal(raw, first)
        rc, _, ar, out = guarded_build(dev, a, levels, 0xA5, H.R_CODE[resampling], nodata, short_by=1)
        assert rc == pyramid.E_ARG and b"levels need" in pyramid.lib().lbdrn_pyr_last_error()
        ar.check()
        assert bool((out.as_u8() == 0xA5).all())      # nothing was launched
    # the binding on a stream of the caller's
    t = to_device(a, dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got = pyramid.build(t, levels, resampling, nodata, stream=side)
    side.synchronize()
    assert_levels(got, want, "stream")


# ---------------------------------------------------------------- files

@pytest.mark.parametrize("shape", ((8, 75, 130), (2, 37, 53)), ids=H.shape_id)
def test_round_trip_through_a_pyramidal_file(dev, shape, tmp_path):
    from lbdrn_hip import raster_io, tiff
    a = TW.base_raster(*shape)
    t = to_device(a, dev)
    path, plain = str(tmp_path / "p.tif"), str(tmp_path / "plain.tif")
    raster_io.write_raster_device(plain, t, tile=16)
    raster_io.write_raster_device(path, t, tile=16, overviews="auto", geo=H.GEO)
    sizes = R.level_sizes(*shape[1:], "auto", 16)
    want = R.pyramid(a, len(sizes))
    assert len(sizes) == (4 if shape[1] == 75 else 2)
    buf = open(path, "rb").read()
    assert len(tiff.read_ifds(buf)) == len(sizes) + 1 and tiff.overview_ifds(buf) == list(range(1, len(sizes) + 1))
    for k, w in enumerate(want, 1):
        got = raster_io.read_raster_device(path, overview=k)
        assert got.is_cuda and np.array_equal(to_host(got), w), k
        assert np.array_equal(raster_io.read_raster(path, overview=k), w)
    assert np.array_equal(to_host(raster_io.read_raster_device(path, overview=0)), a)
    assert np.array_equal(to_host(raster_io.read_raster_device(path)), a)
    assert np.array_equal(raster_io.read_raster(path), a) and np.array_equal(raster_io.read_raster(plain), a)
    with pytest.raises(IndexError, match=f"has {len(sizes)} overview levels"):
        raster_io.read_raster_device(path, overview=len(sizes) + 1)
    with pytest.raises(IndexError, match="has 0 overview levels"):
        raster_io.read_raster(plain, overview=1)
    assert raster_io.read_geo_tags(path) == H.GEO and raster_io.read_geo_tags(plain) == []
    # level 0's segments are the plain file's, byte for byte, at the file's end
    sc0, scp = tiff.parse(buf), tiff.parse(open(plain, "rb").read())
    body = open(plain, "rb").read()[int(scp.offsets[0]):]
    assert buf.endswith(body) and sc0.counts.tolist() == scp.counts.tolist()
    # without the new options the file is what it always was
    again = str(tmp_path / "again.tif")
    raster_io.write_raster_device(again, t, tile=16, overviews=None, resampling="average", nodata=None, geo=None)
    assert open(again, "rb").read() == open(plain, "rb").read()
    # a count, nearest, nodata, from a view of a larger scene, through write_raster too
    view = t[:, 3:3 + 30, 5:5 + 41]
    crop = np.ascontiguousarray(a[:, 3:33, 5:46])
    raster_io.write_raster_device(path, view, tile=16, overviews=3, nodata=513)
    for k, w in enumerate(R.pyramid(crop, 3, "average", 513), 1):
        assert np.array_equal(raster_io.read_raster(path, overview=k), w)
    raster_io.write_raster(path, crop, compress="deflate", tile=16, overviews=2, resampling="nearest")
    for k, w in enumerate(R.pyramid(crop, 2, "nearest"), 1):
        assert np.array_equal(raster_io.read_raster(path, overview=k), w)
    assert np.array_equal(raster_io.read_raster(path), crop)


def test_pillow_reads_every_frame_of_a_one_band_file(dev, tmp_path):
    from lbdrn_hip import raster_io
    try:
        from PIL import Image
    except Exception as e:      # noqa: BLE001
        pytest.skip(f"Pillow does not import: {e}")
    for a in (TW.base_raster(C=1, H=75, W=130), TW.base_raster(C=1, H=75, W=130, dtype=np.uint8)):
        path = str(tmp_path / "one.tif")
        raster_io.write_raster_device(path, to_device(a, dev), tile=16, overviews="auto")
        want = [a] + R.pyramid(a, 4)
        try:
            with Image.open(path) as im:
                assert im.n_frames == 5
                for k in range(5):
                    im.seek(k)
                    assert np.array_equal(np.asarray(im), want[k][0]), k
        except Exception as e:      # noqa: BLE001
            if "decoder" in str(e) and "not available" in str(e):
                pytest.skip(f"this Pillow has no libtiff: {e}")
            raise


# ---------------------------------------------------------------- the command lines

def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f if "Time elapsed" not in line]


@pytest.fixture(scope="module")
def streams(tmp_path_factory, dev):
    """two small .bin files (the shapes of tests/test_gpu_tiff_write.py): one image, -sr 1; four tiles with a lossless residual
    layer, -sr 2"""
    import encode
    from lbdrn_hip.synth import synthetic_tile
    root = tmp_path_factory.mktemp("pyramid_cli")
    saved = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = {}
    try:
        for name, shape, flags in (("one", (8, 40, 52), ["-K", "5", "-D", "2", "-bc", "64", "-nl", "2", "-sr", "1"]),
                                   ("layered", (4, 50, 37), ["-D", "1", "-sr", "2", "--max-error", "0"])):
            img = synthetic_tile(3 + len(name), *shape)
            src = str(root / f"{name}.npy")
            np.save(src, img)
            assert encode.main(["-i", src, "-o", str(root / name), "-e", "1", "-bs", "512"] + flags) == 0
            (sub,) = [d for d in (root / name).iterdir() if d.is_dir()]
            out[name] = (img, src, sub, str(sub / f"{name}.bin"))
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return out


def _check_levels(path, level0, nodata=None, resampling="average"):
    from lbdrn_hip import raster_io
    sizes = R.level_sizes(*level0.shape[1:], "auto", 16)
    assert len(sizes) >= 1
    for k, w in enumerate(R.pyramid(level0, len(sizes), resampling, nodata), 1):
        assert np.array_equal(raster_io.read_raster(path, overview=k), w), k
    with pytest.raises(IndexError):
        raster_io.read_raster(path, overview=len(sizes) + 1)


@pytest.mark.parametrize("name", ("one", "layered"))
def test_decode_out_overviews_adds_the_levels_and_changes_nothing_else(dev, streams, name, tmp_path, monkeypatch):
    """-sr 1 ("one") and -sr 2 ("layered"), whole and --window: level 0 is the raster of the run without the flag, every level
    the reference of that level 0, the records those of the run without the flag; --out-georef puts a file's tags on the output"""
    import decode
    from lbdrn_hip import raster_io
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    img, src, sub, bin_path = streams[name]
    recon, log, wlog = str(sub / f"{name}_recon.tif"), str(sub / "decode.txt"), str(sub / "decode_window.txt")
    georef = str(tmp_path / "georef.tif")
    with open(georef, "wb") as f:
        f.write(H.with_tags(TW.R.write_tiff(img[:1, :8, :8])[0], H.GEO))
    base = ["--out-compress", "deflate", "--out-tile", "16"]
    x0, y0, w, h = 5, 7, 30, 21

    def run(extra, window, org=False):
        for p in (recon, log, wlog):
            if os.path.exists(p):
                os.remove(p)
        wout = str(tmp_path / "w.tif")
        argv = ["-i", bin_path] + (["-org", src] if org else []) + (["--window", str(x0), str(y0), str(w), str(h), "-o", wout] if window else [])
        assert decode.main(argv + base + extra) == 0
        return (wout if window else recon), _records(wlog if window else log)
    for window in (False, True):
        path, plain_records = run([], window)
        level0 = raster_io.read_raster(path)
        plain_bytes = open(path, "rb").read()
        assert raster_io.read_geo_tags(path) == []
        path, records = run(["--out-overviews", "auto"], window)
        assert records == plain_records
        assert np.array_equal(raster_io.read_raster(path), level0)      # sample for sample
        _check_levels(path, level0)
        assert open(path, "rb").read() != plain_bytes and raster_io.read_geo_tags(path) == []
        path, records = run(["--out-overviews", "auto", "--out-resampling", "nearest", "--out-georef", georef], window)
        assert records == plain_records and raster_io.read_geo_tags(path) == H.GEO
        _check_levels(path, level0, resampling="nearest")
        path, records = run(["--out-overviews", "1", "--out-nodata", str(int(level0[0, 0, 0]))], window)
        assert records == plain_records and np.array_equal(raster_io.read_raster(path), level0)
        assert np.array_equal(raster_io.read_raster(path, overview=1), R.reduce_level(level0, "average", int(level0[0, 0, 0])))
        path, records = run(["--out-georef", georef], window)
        assert records == plain_records and raster_io.read_geo_tags(path) == H.GEO and np.array_equal(raster_io.read_raster(path), level0)
        with pytest.raises(IndexError, match="has 0 overview"):
            raster_io.read_raster(path, overview=1)
    # with -org the records are those of the run without the flag (the raster is removed behind them)
    a, b = run([], False, org=True)[1], run(["--out-overviews", "auto"], False, org=True)[1]
    assert a == b and any(r.startswith("PSNR") for r in a)
    if name == "layered":
        assert np.array_equal(level0, img[:, y0:y0 + h, x0:x0 + w])      # --max-error 0: the window of the original


def test_converter_in_a_child_process(dev, tmp_path):
    """python -m lbdrn_hip.pyramid on an LZW file of one-row strips with georeferencing tags"""
    from lbdrn_hip import raster_io, tiff
    a = TW.base_raster(C=3, H=75, W=130)
    src, dst = str(tmp_path / "in.tif"), str(tmp_path / "out.tif")
    with open(src, "wb") as f:
        f.write(H.with_tags(TW.R.write_tiff(a, rows_per_strip=1, compression=TW.R.COMP_LZW, predictor=2)[0], H.GEO))
    env = dict(os.environ, PYTHONPATH=os.path.join(H.ROOT, "lbdrn-msic_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def child(*args):
        return subprocess.run([sys.executable, "-m", "lbdrn_hip.pyramid"] + list(args), capture_output=True, text=True, env=env, timeout=300)
    run = child(src, dst, "--tile", "16")
    assert run.returncode == 0, run.stderr
    assert np.array_equal(raster_io.read_raster(dst), a) and raster_io.read_geo_tags(dst) == H.GEO
    lay = tiff.parse(open(dst, "rb").read()).layout
    assert (lay.tiled, lay.seg_w, lay.compression, lay.predictor) == (1, 16, 8, 2)
    for k, w in enumerate(R.pyramid(a, 4), 1):
        assert np.array_equal(raster_io.read_raster(dst, overview=k), w)
    run = child(src, dst, "--tile", "16", "--overviews", "2", "--resampling", "nearest", "--nodata", "513", "--no-georef")
    assert run.returncode == 0, run.stderr
    assert raster_io.read_geo_tags(dst) == [] and len(tiff.read_ifds(open(dst, "rb").read())) == 3
    for k, w in enumerate(R.pyramid(a, 2, "nearest"), 1):
        assert np.array_equal(raster_io.read_raster(dst, overview=k), w)
    run = child(src, dst, "--tile", "16", "--overviews", "9")
    assert run.returncode == 2 and "1 x 1" in run.stderr
