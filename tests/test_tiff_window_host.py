"""Reading a window of a scene, the host side: tiff.plan_window against a brute-force statement over every layout the reader
takes, that nothing outside the plan's byte ranges is read, the window reads of raster_io that need no device, raster_shape,
the refusals, and encode.py --window / LBDRN_TILE_READS=1 with the GPU work replaced by stand-ins (as
tests/test_resid_sharding_cpu.py does).  The decompression on the device is stood in for by tests/tiff_reference.py, which
decodes the sub-layout the library would be handed: the plan is checked to describe a scene that stands by itself."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tiff_reference as R  # noqa: E402
from test_cli_sharding_cpu import _records, _stub_report, _stub_train_tiles  # noqa: E402

H, W = 53, 37
LAYOUTS = [dict(tile=(16, 16)), dict(tile=(32, 16)), dict(rows_per_strip=1), dict(rows_per_strip=5), dict(rows_per_strip=37),
           dict(rows_per_strip=None)]
WINDOWS = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),      # the four corners
           (17, 18, 5, 6),          # inside one tile of either size
           (28, 10, 8, 12),         # across x = 32 and y = 16: four tiles of either size
           (5, 51, 10, 2),          # inside the short last strip of 5-row strips (rows 50..52)
           (33, 49, 3, 3),          # inside the bottom right edge tile (x 32..36, y 48..52)
           (0, 0, W, H)]


def _image(C, dtype=np.uint16, seed=0):
    rng = np.random.default_rng(seed)
    smooth = (np.arange(H)[:, None] * 7 + np.arange(W)[None, :] * 3)[None] + 100 * np.arange(C)[:, None, None]
    return (smooth + rng.integers(0, 4, (C, H, W))).astype(dtype) * (1 if dtype == np.uint8 else 150)


def _touched(C, lay_kw, planar, window):
    """brute force: every segment's rectangle inside the image, intersected with the window -> (indices, bounding box)"""
    x0, y0, w, h = window
    idx, box = [], [H, W, 0, 0]
    for i, (b, sy, sx, sh, sw, rows) in enumerate(R.segment_grid(C, H, W, lay_kw.get("tile"), lay_kw.get("rows_per_strip"), planar)):
        ey, ex = sy + rows, min(sx + sw, W)
        if sy < y0 + h and y0 < ey and sx < x0 + w and x0 < ex:
            idx.append(i)
            box = [min(box[0], sy), min(box[1], sx), max(box[2], ey), max(box[3], ex)]
    return idx, box


def _check_plan(tiff, data, scene, lay_kw, planar, C, window):
    plan = tiff.plan_window(scene, window)
    idx, (by0, bx0, by1, bx1) = _touched(C, lay_kw, planar, window)
    assert list(plan.segments) == idx      # the set, and TIFF order over the sub-grid is ascending order in the file's table
    lay, full = plan.layout, scene.layout
    assert (lay.C, lay.H, lay.W) == (C, by1 - by0, bx1 - bx0)
    assert plan.crop == (window[1] - by0, window[0] - bx0)
    for name in ("bits", "big_endian", "planar", "tiled", "compression", "predictor", "seg_w"):
        assert getattr(lay, name) == getattr(full, name), name
    assert lay.seg_h == (full.seg_h if full.tiled else min(full.seg_h, lay.H))
    assert tiff.lib().lbdrn_tiff_segment_count(ctypes.byref(lay)) == len(plan.segments)
    # ranges: sorted, disjoint, neighbours merged; nbytes their sum; the rebased table points at the same bytes
    ends = [o + n for o, n in plan.ranges]
    assert all(n > 0 for _, n in plan.ranges) and all(e < o for e, (o, _) in zip(ends, plan.ranges[1:]))
    assert plan.nbytes == sum(n for _, n in plan.ranges)
    compact = bytes(plan.gather(data))
    assert len(compact) == plan.nbytes
    for k, i in enumerate(plan.segments):
        o, c = int(plan.offsets[k]), int(plan.counts[k])
        assert c == int(scene.counts[i]) and o + c <= plan.nbytes
        assert compact[o:o + c] == data[int(scene.offsets[i]):int(scene.offsets[i]) + c]
    return plan


@pytest.mark.parametrize("C", [1, 3, 8])
def test_plan_window_against_brute_force(C):
    from lbdrn_hip import tiff
    a = _image(C)
    for lay_kw, planar, big, bo in itertools.product(LAYOUTS, (1, 2), (False, True), "<>"):
        data, _ = R.write_tiff(a, bigtiff=big, byteorder=bo, planar=planar, **lay_kw)
        scene = tiff.parse(data)
        for window in WINDOWS:
            _check_plan(tiff, data, scene, lay_kw, planar, C, window)


def test_plan_of_the_short_last_strip_and_of_an_edge_tile():
    from lbdrn_hip import tiff
    a = _image(3)
    scene = tiff.parse(R.write_tiff(a, rows_per_strip=5, planar=2)[0])
    plan = tiff.plan_window(scene, (5, 51, 10, 2))
    assert plan.segments == [10, 21, 32] and (plan.layout.H, plan.layout.seg_h, plan.layout.W) == (3, 3, W) and plan.crop == (1, 5)
    scene = tiff.parse(R.write_tiff(a, tile=(16, 16), planar=1)[0])
    plan = tiff.plan_window(scene, (33, 49, 3, 3))
    assert plan.segments == [11] and (plan.layout.H, plan.layout.W, plan.layout.seg_h, plan.layout.seg_w) == (5, 5, 16, 16)
    assert plan.crop == (1, 1)


# ---------------------------------------------------------------- nothing else is read

class Recording:
    """a file that has len() and slices, and remembers every byte it gave out"""

    def __init__(self, data):
        self.data, self.seen = data, np.zeros(len(data), bool)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, key):
        self.seen[key] = True
        return self.data[key]


def _host_decode(buf, scene, dev):
    """Stands where tiff.decode_device stands: the scene it is handed -- a window's sub-layout over its compact buffer --
    decoded by tests/tiff_reference.py"""
    lay = scene.layout
    dt = np.uint8 if lay.bits == 8 else np.uint16
    tile = (lay.seg_w, lay.seg_h) if lay.tiled else None
    grid = R.segment_grid(lay.C, lay.H, lay.W, tile, None if lay.tiled else lay.seg_h, lay.planar)
    assert len(grid) == len(scene.offsets)
    spp = lay.C if lay.planar == 1 else 1
    segs = []
    for (b, y0, x0, sh, sw, rows), o, c in zip(grid, scene.offsets, scene.counts):
        expect = (sh if lay.tiled else rows) * sw * spp * (lay.bits // 8)
        segs.append(R.decompress(bytes(buf[int(o):int(o) + int(c)]), lay.compression, expect))
    a = R.place_segments(segs, lay.C, lay.H, lay.W, dt, tile, None if lay.tiled else lay.seg_h, lay.planar, lay.predictor,
                         ">" if lay.big_endian else "<")
    return torch.from_numpy(a.view(np.int16) if dt == np.uint16 else a)


def _allowed(tiff, data, plan):
    """the header, everything from the first IFD on (tests/tiff_reference.py writes the IFD and the tag arrays behind the
    segments) and the plan's ranges"""
    ok = np.zeros(len(data), bool)
    ok[:16] = True
    ok[tiff.read_ifds(data)[0]:] = True
    for o, n in plan.ranges:
        ok[o:o + n] = True
    return ok


@pytest.mark.parametrize("comp", [R.COMP_NONE, R.COMP_LZW, R.COMP_DEFLATE, R.COMP_PACKBITS])
def test_a_window_read_touches_only_its_plan(comp, monkeypatch):
    from lbdrn_hip import tiff
    monkeypatch.setattr(tiff, "decode_device", _host_decode)
    monkeypatch.setattr(tiff, "_device", lambda device: "cpu")
    for C, lay_kw, planar, big, pred in ((8, dict(tile=(16, 16)), 2, False, 2), (3, dict(tile=(32, 16)), 1, True, 1),
                                         (3, dict(rows_per_strip=5), 1, False, 2), (1, dict(rows_per_strip=1), 2, True, 1)):
        a = _image(C)
        data, _ = R.write_tiff(a, bigtiff=big, planar=planar, predictor=pred, compression=comp, **lay_kw)
        scene = tiff.parse(data)
        for window in WINDOWS[:-1]:
            x0, y0, w, h = window
            rec = Recording(data)
            got = tiff.read_window_bytes(rec, "scene.tif", window)
            got = got.numpy().view(np.uint16)
            assert got.shape == (C, h, w) and np.array_equal(got, a[:, y0:y0 + h, x0:x0 + w]), (comp, lay_kw, window)
            plan = tiff.plan_window(scene, window)
            assert not (rec.seen & ~_allowed(tiff, data, plan)).any(), (comp, lay_kw, window)
            assert rec.seen.sum() < len(data)
            if C == 8 and window == (0, 0, 1, 1):      # eight tiles that are no neighbours in the file: not a byte more
                assert len(plan.segments) == 8 and plan.nbytes == sum(int(scene.counts[i]) for i in plan.segments)


def test_a_damaged_segment_outside_the_window_is_not_looked_at(monkeypatch):
    from lbdrn_hip import tiff
    monkeypatch.setattr(tiff, "decode_device", _host_decode)
    monkeypatch.setattr(tiff, "_device", lambda device: "cpu")
    a = _image(3)
    # old-style LZW in segment 13: the whole file is refused by the parser, a window elsewhere reads
    data, _ = R.write_tiff(a, tile=(16, 16), planar=2, compression=R.COMP_LZW,
                           segment_hook=lambda i, p: b"\0\1" + p[2:] if i == 13 else p)
    with pytest.raises(ValueError, match="segment 13 is old-style"):
        tiff.parse(data)
    got = tiff.read_window_bytes(data, "scene.tif", (0, 0, 16, 16)).numpy().view(np.uint16)
    assert np.array_equal(got, a[:, :16, :16])
    with pytest.raises(ValueError, match="segment 13 is old-style"):
        tiff.read_window_bytes(data, "scene.tif", (16, 0, 4, 4))      # band 1's tile (0, 1) is segment 13


def test_the_host_route_of_over_cap_deflate_inflates_the_touched_strips_only(monkeypatch):
    from lbdrn_hip import tiff
    a = _image(3)
    data, _ = R.write_tiff(a, rows_per_strip=5, planar=1, predictor=2, compression=R.COMP_DEFLATE,
                           segment_hook=lambda i, p: p[:4] if i == 0 else p)      # strip 0 is damaged
    monkeypatch.setattr(tiff, "_over_cap", lambda lay, path: "host")
    monkeypatch.setattr(tiff, "_device", lambda device: pytest.fail("the host route needs no device"))
    scene = tiff.parse(data)
    rec = Recording(data)
    got = tiff._window(rec, "scene.tif", (3, 7, 20, 30), None, 0, False)
    assert got.dtype == np.uint16 and np.array_equal(got, a[:, 7:37, 3:23])
    assert not (rec.seen & ~_allowed(tiff, data, tiff.plan_window(scene, (3, 7, 20, 30)))).any()
    with pytest.raises(tiff.TiffError, match="segment 0 is damaged"):
        tiff._window(data, "scene.tif", (0, 4, 5, 5), None, 0, False)
    # the names are the file's: the second strip touched is the sub-layout's segment 1 and the file's segment 3
    data, _ = R.write_tiff(a, rows_per_strip=5, planar=1, compression=R.COMP_DEFLATE, segment_hook=lambda i, p: p[:4] if i == 3 else p)
    with pytest.raises(tiff.TiffError, match="segment 3 is damaged"):
        tiff._window(data, "scene.tif", (0, 12, 5, 5), None, 0, False)


# ---------------------------------------------------------------- raster_io without a device

def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_plain_strips_and_npy_windows_equal_the_slice(dtype, tmp_path):
    from lbdrn_hip import raster_io
    a = _image(3, np.uint16 if dtype == np.float32 else dtype).astype(dtype)
    if dtype == np.float32:
        a = a / 7
    paths = [str(tmp_path / "own.tif"), str(tmp_path / "a.npy"), str(tmp_path / "one.tif"), str(tmp_path / "one.npy")]
    raster_io.write_raster(paths[0], a)
    np.save(paths[1], a)
    raster_io.write_raster(paths[2], a[:1])
    np.save(paths[3], a[0])
    if dtype != np.float32:      # several strips, chunky, big-endian; rows of one strip; a strip per row
        paths.append(_write(tmp_path / "chunky.tif", R.write_tiff(a, rows_per_strip=5, planar=1, byteorder=">")[0]))
        paths.append(_write(tmp_path / "planar.tif", R.write_tiff(a, rows_per_strip=1, planar=2)[0]))
    for path in paths:
        full = raster_io.read_raster(path)
        C = 1 if full.ndim == 2 else full.shape[0]
        assert raster_io.raster_shape(path) == (C, H, W, np.dtype(dtype))
        for x0, y0, w, h in WINDOWS:
            got = raster_io.read_raster(path, window=(x0, y0, w, h))
            want = full[..., y0:y0 + h, x0:x0 + w]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (path, x0, y0, w, h)


def test_a_plain_strip_window_reads_its_rows_only(tmp_path):
    from lbdrn_hip import raster_io, tiff
    a = _image(3)
    data, _ = R.write_tiff(a, rows_per_strip=5, planar=2)
    rec = Recording(data)
    got = raster_io._window_of_strips(rec, raster_io._classic_plain(rec), (4, 11, 9, 13))
    assert np.array_equal(got, a[:, 11:24, 4:13])
    plan = tiff.plan_window(tiff.parse(data), (4, 11, 9, 13))
    assert not (rec.seen & ~_allowed(tiff, data, plan)).any()
    assert rec.seen[8:tiff.read_ifds(data)[0]].sum() == 3 * 13 * W * 2      # the window's rows of each band
    rec = Recording(data)      # the same through lbdrn_hip.tiff, which takes BigTIFF strips too
    assert np.array_equal(tiff._window(rec, "scene.tif", (4, 11, 9, 13), None, 0, False), a[:, 11:24, 4:13])
    assert rec.seen[8:tiff.read_ifds(data)[0]].sum() == 3 * 13 * W * 2


def test_raster_shape_reads_the_tags_of_every_file_kind(tmp_path):
    from lbdrn_hip import raster_io
    a8, a16 = _image(3, np.uint8), _image(8)
    cases = [(_write(tmp_path / "tiled.tif", R.write_tiff(a16, tile=(16, 16), compression=R.COMP_DEFLATE, predictor=2)[0]), (8, H, W, np.uint16)),
             (_write(tmp_path / "big.tif", R.write_tiff(a8, bigtiff=True, byteorder=">", rows_per_strip=5, compression=R.COMP_LZW)[0]), (3, H, W, np.uint8)),
             (_write(tmp_path / "bigplain.tif", R.write_tiff(a16[:1], bigtiff=True)[0]), (1, H, W, np.uint16)),
             (_write(tmp_path / "packbits.tif", R.write_tiff(a8[:1], compression=R.COMP_PACKBITS)[0]), (1, H, W, np.uint8))]
    for path, want in cases:
        assert raster_io.raster_shape(path) == want[:3] + (np.dtype(want[3]),)
    with pytest.raises(IndexError, match="overview 1 of a file that has 0"):
        raster_io.raster_shape(cases[0][0], overview=1)
    with pytest.raises(IndexError):
        raster_io.raster_shape(str(tmp_path / "a.npy"), overview=1)
    # no pixel data: a file cut behind its tags still tells its shape
    data = R.write_tiff(a16, tile=(16, 16))[0]
    rec = Recording(data)
    from lbdrn_hip import tiff
    assert tiff._parse(rec, "x", 0, False).shape == (8, H, W) and not rec.seen[16:tiff.read_ifds(data)[0]].any()


def test_windows_outside_the_raster_are_refused_in_check_window_s_words(tmp_path):
    from lbdrn_hip import codec, raster_io, tiff
    a = _image(3)
    tif, npy = str(tmp_path / "a.tif"), str(tmp_path / "a.npy")
    raster_io.write_raster(tif, a)
    np.save(npy, a)
    tiled = R.write_tiff(a, tile=(16, 16), compression=R.COMP_LZW)[0]
    for window in ((0, 0, 0, 5), (3, 3, 5, -1), (-1, 0, 4, 4), (0, -2, 4, 4), (30, 0, 8, 4), (0, 50, 4, 4), (0, 0, W + 1, H), (1, 2, 3)):
        with pytest.raises(ValueError) as want:
            codec.check_window(window, W, H)
        for read in (lambda: raster_io.read_raster(tif, window=window), lambda: raster_io.read_raster(npy, window=window),
                     lambda: tiff.plan_window(tiff.parse(tiled), window), lambda: tiff.read_window_bytes(tiled, "t.tif", window)):
            with pytest.raises(ValueError) as got:
                read()
            assert str(got.value) == str(want.value)


def test_a_read_without_a_window_is_the_read_it_was(tmp_path):
    from lbdrn_hip import raster_io
    a = _image(3)
    for path in (str(tmp_path / "a.tif"), str(tmp_path / "a.npy")):
        raster_io.write_raster(path, a)
        for got in (raster_io.read_raster(path), raster_io.read_raster(path, window=None), raster_io.read_raster(path, 0, None),
                    raster_io.read_raster(path, window=(0, 0, W, H))):
            assert got.dtype == a.dtype and np.array_equal(got, a)
        assert type(raster_io.read_raster(path)) is np.ndarray and raster_io.raster_size(path) == (W, H)


# ---------------------------------------------------------------- encode.py --window and LBDRN_TILE_READS=1

ARGS = ["-sr", "2", "-K", "4", "-e", "2", "-bs", "64"]
WIN = (5, 7, 30, 41)
STEM = "scene_x5_y7_w30_h41"
SUB = "_r2_K4_bc64_nl2_D2_prec16_lr0.001_bs64_e2"


def _encode_worker(rank, world, port, argv, tile_reads):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    os.environ["LBDRN_TILE_READS"] = "1" if tile_reads else "0"
    import encode
    encode.train_tiles, encode.report_and_pack = _stub_train_tiles, _stub_report
    assert encode.main(argv) == 0


def _strip(records, *roots):
    out = []
    for r in records:
        if r.startswith("Time elapsed"):
            continue
        for root in roots:
            r = r.replace(str(root), "X")
        out.append(r)
    return out


@pytest.mark.parametrize("ext", ["npy", "tif"])
def test_encode_window_and_tile_reads_write_the_bin_of_the_cropped_file(ext, tmp_path, monkeypatch):
    import encode
    from lbdrn_hip import container, raster_io
    img = _image(2, seed=4)
    x0, y0, w, h = WIN
    src, crop = str(tmp_path / f"scene.{ext}"), str(tmp_path / f"{STEM}.{ext}")
    raster_io.write_raster(src, img)
    raster_io.write_raster(crop, np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w]))
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBDRN_TILE_READS"):
        monkeypatch.delenv(k, raising=False)
    win = ["--window"] + [str(v) for v in WIN]
    assert encode.main(["-i", crop, "-o", str(tmp_path / "crop")] + ARGS) == 0
    assert encode.main(["-i", src, "-o", str(tmp_path / "window")] + ARGS + win) == 0
    assert encode.main(["-i", src, "-o", str(tmp_path / "whole")] + ARGS) == 0
    # with a (stand-in) residual layer, which is coded against the tile's pixels: the trailer of the crop's file
    from test_resid_sharding_cpu import _stub_layer
    monkeypatch.setattr(encode, "residual_layer", _stub_layer)
    assert encode.main(["-i", crop, "-o", str(tmp_path / "crop_layer"), "--max-error", "3"] + ARGS) == 0
    assert encode.main(["-i", src, "-o", str(tmp_path / "window_layer"), "--max-error", "3"] + ARGS + win) == 0
    layered = (tmp_path / "crop_layer" / (STEM + SUB) / f"{STEM}.bin").read_bytes()
    assert (tmp_path / "window_layer" / (STEM + SUB) / f"{STEM}.bin").read_bytes() == layered
    assert container.unpack_residual_trailer(layered)[0] == 3
    monkeypatch.setenv("LBDRN_TILE_READS", "1")
    assert encode.main(["-i", src, "-o", str(tmp_path / "window_layer_tiles"), "--max-error", "3"] + ARGS + win) == 0
    assert (tmp_path / "window_layer_tiles" / (STEM + SUB) / f"{STEM}.bin").read_bytes() == layered
    whole_reads = []
    monkeypatch.setattr(raster_io, "read_raster", lambda path, overview=0, window=None, _read=raster_io.read_raster:
                        (whole_reads.append(path) if window is None else None, _read(path, overview, window))[1])
    assert encode.main(["-i", src, "-o", str(tmp_path / "window_tiles")] + ARGS + win) == 0
    assert encode.main(["-i", src, "-o", str(tmp_path / "whole_tiles")] + ARGS) == 0
    assert whole_reads == []      # the scene is never held: every read was a tile's window
    monkeypatch.undo()
    port = 29350 + os.getpid() % 200
    sharded = (("window_sharded", False), ("window_tiles_sharded", True)) if ext == "tif" else ()      # two gloo ranks, once
    for k, (name, reads) in enumerate(sharded):
        argv = ARGS + win
        mp.spawn(_encode_worker, args=(2, port + k, ["-i", src, "-o", str(tmp_path / name)] + argv, reads), nprocs=2, join=True)
    want = (tmp_path / "crop" / (STEM + SUB) / f"{STEM}.bin").read_bytes()
    assert container.unpack_header(want)[1:4] == (2, w, h) and len(want) > 4 * 64
    for name in ("window", "window_tiles") + tuple(name for name, _ in sharded):
        assert (tmp_path / name / (STEM + SUB) / f"{STEM}.bin").read_bytes() == want, name
        got = _strip(_records(tmp_path / name / (STEM + SUB) / "encode.txt"), tmp_path / name)
        assert [r for r in got if r.startswith(("nn: ", "MSB: "))] == \
            [r for r in _strip(_records(tmp_path / "crop" / (STEM + SUB) / "encode.txt")) if r.startswith(("nn: ", "MSB: "))]
    whole = (tmp_path / "whole" / ("scene" + SUB) / "scene.bin").read_bytes()
    assert container.unpack_header(whole)[2:4] == (W, H) and whole != want
    for name in ("whole_tiles",):
        assert (tmp_path / name / ("scene" + SUB) / "scene.bin").read_bytes() == whole, name
    # LBDRN_TILE_READS changes no record but the times
    assert _strip(_records(tmp_path / "whole_tiles" / ("scene" + SUB) / "encode.txt"), tmp_path / "whole_tiles") == \
        _strip(_records(tmp_path / "whole" / ("scene" + SUB) / "encode.txt"), tmp_path / "whole")
    assert _strip(_records(tmp_path / "window_tiles" / (STEM + SUB) / "encode.txt"), tmp_path / "window_tiles") == \
        _strip(_records(tmp_path / "window" / (STEM + SUB) / "encode.txt"), tmp_path / "window")


def test_encode_refuses_a_window_outside_the_scene(tmp_path, capsys):
    import encode
    src = str(tmp_path / "scene.npy")
    np.save(src, _image(2))
    with pytest.raises(SystemExit) as e:
        encode.main(["-i", src, "-o", str(tmp_path / "out"), "--window", "30", "0", "8", "4"] + ARGS)
    assert e.value.code == 2 and f"is not inside the {W} x {H} scene" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
    a = encode.build_parser().parse_args(["-i", src])
    assert not hasattr(a, "window") and encode.scene_name(a) == "scene"      # a run without --window logs the arguments it always logged


def test_main_k_points_and_the_sweep_pass_the_window_through(tmp_path, monkeypatch):
    """main_k_points with --window, and with LBDRN_TILE_READS=1, writes what main() writes point after point; sweep.py hands
    the window to encode.py and tells decode.py that the original is that part of the file"""
    import encode
    import sweep
    from lbdrn_hip import raster_io
    from test_sweep_in_flight_host import _stub_train_tiles as tiles_k, _stub_train_tiles_at
    src = str(tmp_path / "scene.tif")
    raster_io.write_raster(src, _image(2, seed=4))
    monkeypatch.setattr(encode, "train_tiles", tiles_k)
    monkeypatch.setattr(encode, "train_tiles_at", _stub_train_tiles_at)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    monkeypatch.setattr(encode, "BASE_CODEC", "LBB2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBDRN_TILE_READS"):
        monkeypatch.delenv(k, raising=False)
    common = ARGS[:2] + ARGS[4:] + ["--window"] + [str(v) for v in WIN]
    Ks = (3, 4)
    for K in Ks:
        assert encode.main(["-i", src, "-o", str(tmp_path / "one"), "-K", str(K)] + common, shard_tiles=False) == 0
    assert encode.main_k_points(["-i", src, "-o", str(tmp_path / "many")] + common, Ks) == {K: None for K in Ks}
    monkeypatch.setenv("LBDRN_TILE_READS", "1")
    assert encode.main_k_points(["-i", src, "-o", str(tmp_path / "many_tiles")] + common, Ks) == {K: None for K in Ks}
    for K in Ks:
        sub = STEM + SUB.replace("K4", f"K{K}")
        want = (tmp_path / "one" / sub / f"{STEM}.bin").read_bytes()
        for name in ("many", "many_tiles"):
            assert (tmp_path / name / sub / f"{STEM}.bin").read_bytes() == want, (name, K)
            assert _strip(_records(tmp_path / name / sub / "encode.txt"), tmp_path / name) == \
                _strip(_records(tmp_path / "one" / sub / "encode.txt"), tmp_path / "one")
    a = sweep.parse(["--images", src, "--k", "3", "4", "-sr", "2", "-e", "2", "-bs", "64", "-o", str(tmp_path / "one"), "--window"] +
                    [str(v) for v in WIN])
    assert sweep.common_args(a)[-5:] == ["--window", "5", "7", "30", "41"] and sweep.point_stem(a, src) == STEM
    assert sweep.point_folder(a, src, 4) == str(tmp_path / "one" / (STEM + SUB))
    calls = []
    monkeypatch.setattr(sweep.decode, "main", lambda argv, shard_tiles=None: calls.append(argv))
    sweep.decode_point(a, src, 4)
    assert calls == [["-i", str(tmp_path / "one" / (STEM + SUB) / f"{STEM}.bin"), "-org", src, "--org-window", "5", "7", "30", "41"]]
    plain = sweep.parse(["--images", src])
    assert "--window" not in sweep.common_args(plain) and sweep.point_stem(plain, src) == "scene"


def test_decode_org_window_compares_with_that_part_of_the_original(tmp_path, monkeypatch):
    """the whole decode of a file that encode.py --window wrote: -org names the scene, --org-window the part that was encoded;
    the records are those of comparing with a file that holds the crop (stand-ins as tests/test_cli_sharding_cpu.py has them)"""
    import decode
    from lbdrn_hip import codec, container
    from test_cli_sharding_cpu import _stub_apply
    nn, base = [b"w" * 10] * 4, [bytes(range(t, t + 48)) + b"pad" * t for t in range(4)]
    blob = container.pack_header(2, 12, 8, 3, 64, 2, 2, [len(x) for x in nn], [len(x) for x in base])
    for x, y in zip(nn, base):
        blob += x + y
    scene = np.random.default_rng(1).integers(0, 2000, (2, 20, 30)).astype(np.uint16)
    np.save(str(tmp_path / "scene.npy"), scene)
    np.save(str(tmp_path / "crop.npy"), np.ascontiguousarray(scene[:, 9:17, 5:17]))
    monkeypatch.setattr(codec, "apply_image", _stub_apply)
    monkeypatch.setattr(container, "decode_weights", lambda payload, expected=None: np.zeros(4, np.float32))
    monkeypatch.setattr(container, "decode_base",
                        lambda payload, device=None, keep_on_device=False: np.frombuffer(payload[:48], np.uint8).reshape(2, 4, 6).copy())
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    outs = []
    for name, extra in (("crop", ["-org", str(tmp_path / "crop.npy")]),
                        ("window", ["-org", str(tmp_path / "scene.npy"), "--org-window", "5", "9", "12", "8"])):
        (tmp_path / name).mkdir()
        (tmp_path / name / "img.bin").write_bytes(blob)
        assert decode.main(["-i", str(tmp_path / name / "img.bin")] + extra) == 0
        outs.append([r for r in _records(tmp_path / name / "decode.txt") if r.startswith(("MSE", "PSNR", "Total size"))])
    assert outs[0] == outs[1] and len(outs[0]) == 3
    with pytest.raises(SystemExit):
        decode.main(["-i", str(tmp_path / "crop" / "img.bin"), "--org-window", "5", "9", "12", "8"])
