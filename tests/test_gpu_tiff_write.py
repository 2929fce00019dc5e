"""Tiled and Deflate-compressed TIFF rasters written through liblbdrn_tiffw.so on the device (csrc/tiffw.hip): every layout
of tests/test_tiff_write_host.py on the 37 x 53 raster, read back by the device reader and compared byte for byte with the
host build of the same text (tests/tiff_write_host_shim.cpp); the encoder's hard segments as one-segment rasters; the size
condition on the golden rasters; the C ABI on guarded buffers under three fills; determinism across runs and streams; and
decode.py --out-compress against decode.py without it.  Every comparison of sample values is exact.

Nothing here ran before the library existed: lbdrn_hip.tiff_write and liblbdrn_tiffw.so are new."""
import ctypes
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_write_helpers as H  # noqa: E402
from guarded import FILLS, Arena  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return H.load_shim(tmp_path_factory)


def to_device(a, dev):
    import torch
    a = np.array(a, order="C")      # (a writable copy: torch wants one)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def device_encode(dev, a, lay):
    from lbdrn_hip import tiff_write
    body, offsets, counts = tiff_write.encode_device(to_device(a, dev), lay)
    return body.tobytes(), offsets.tolist(), counts.tolist()


def explain(dev, shim, a, lay, body, offsets, counts):
    """None where the device's segments equal the host build's byte for byte; else the first differing segment and the stage
    that went wrong: gather (the uncompressed byte image differs), deflate (the coded segment differs), pack (its place)"""
    from lbdrn_hip import tiff_write
    stage = {}
    hbody, hoff, hcnt = H.host_encode(shim, a, lay, stage)
    if body == hbody.tobytes() and offsets == hoff.tolist() and counts == hcnt.tolist():
        return None
    plain = tiff_write.Layout(*[getattr(lay, n) for n, _ in tiff_write.Layout._fields_])
    plain.compression = 1
    pbody, poff, pcnt = device_encode(dev, a, plain)
    for i, raw in enumerate(stage["raw"]):
        if pbody[poff[i]:poff[i] + pcnt[i]] != raw:
            return f"segment {i}: gather"
    for i, coded in enumerate(stage["coded"]):
        if counts[i] != len(coded) or (offsets[i] == hoff[i] and body[offsets[i]:offsets[i] + counts[i]] != coded):
            return f"segment {i}: deflate"
        if offsets[i] != hoff[i]:
            return f"segment {i}: pack"
    return "the total: pack"


# ---------------------------------------------------------------- layouts

@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=("u8", "u16"))
def test_every_layout_reads_back_and_equals_the_host_build(dev, shim, tmp_path, dtype):
    from lbdrn_hip import raster_io, tiff, tiff_write
    path = str(tmp_path / "t.tif")
    full = H.base_raster(dtype=dtype)
    k = 0
    for seg in H.SEGMENTATIONS:
        for planar in (1, 2):
            for compress, pred in H.CODINGS:
                a = np.ascontiguousarray(full[:(1, 3, 4, 8)[k % 4]])
                k += 1
                lay = tiff_write.make_layout(*a.shape, a.dtype.itemsize * 8, compress, planar=planar, predictor=pred, **seg)
                body, offsets, counts = device_encode(dev, a, lay)
                assert explain(dev, shim, a, lay, body, offsets, counts) is None, (seg, planar, compress, pred, a.shape)
                got = tiff_write.write_device(path, to_device(a, dev), compress, planar=planar, predictor=pred, **seg)
                assert [getattr(got, n) for n, _ in tiff_write.Layout._fields_] == [getattr(lay, n) for n, _ in tiff_write.Layout._fields_]
                buf = open(path, "rb").read()
                assert buf.endswith(body) and len(buf) == int(tiff.parse(buf).offsets[0]) + len(body)
                t = raster_io.read_raster_device(path, dev)
                back = t.cpu().numpy()
                back = back.view(np.uint16) if back.dtype == np.int16 else back
                assert back.dtype == a.dtype and np.array_equal(back, a), (seg, planar, compress, pred, a.shape)
    # 8 planar bands of one-row strips: 296 segments, and the same through raster_io from a host array
    a = H.base_raster(dtype=dtype)
    raster_io.write_raster(path, a, compress="deflate", rows_per_strip=1)
    sc = tiff.parse(open(path, "rb").read())
    assert len(sc.offsets) == 296 and sc.layout.predictor == 2
    assert np.array_equal(raster_io.read_raster(path), a)
    raster_io.write_raster_device(path, to_device(a[:1], dev))      # the defaults: Deflate, predictor 2, one 256 x 256 tile
    lay = tiff.parse(open(path, "rb").read()).layout
    assert (lay.tiled, lay.seg_w, lay.seg_h, lay.compression, lay.predictor, lay.planar) == (1, 256, 256, 8, 2, 2)
    assert np.array_equal(raster_io.read_raster(path), a[0])


def test_hard_segments_as_one_segment_rasters(dev, shim, tmp_path):
    from lbdrn_hip import raster_io, tiff_write
    path = str(tmp_path / "s.tif")
    for name, data in H.special_segments(tiff_write.lib().lbdrn_tiffw_block_tokens()).items():
        if len(data) == 131072:      # a 64 x 1024 strip of 16-bit samples is 128 KiB
            a = np.frombuffer(data, "<u2").reshape(1, 64, 1024)
        else:
            a = np.frombuffer(data, np.uint8).reshape(1, 1, -1)
        lay = tiff_write.make_layout(*a.shape, a.dtype.itemsize * 8, "deflate", rows_per_strip=a.shape[1], predictor=1)
        body, offsets, counts = device_encode(dev, a, lay)
        assert offsets == [0] and counts == [len(body)] and len(body) <= tiff_write.lib().lbdrn_tiffw_bound(len(data)), name
        assert zlib.decompress(body) == data, name
        assert body == H.shim_deflate(shim, data)[0], name
        tiff_write.write_device(path, to_device(a, dev), "deflate", rows_per_strip=a.shape[1], predictor=1)
        assert np.array_equal(raster_io.read_raster(path).reshape(a.shape), a), name


def test_size_against_zlib_on_the_golden_rasters(dev, shim, capsys):
    from lbdrn_hip import tiff_write
    for name, tile, recorded in H.GOLDEN_SETUPS:
        img = H.golden_planes(name)
        lay = tiff_write.make_layout(*img.shape, 16, "deflate", tile=tile)
        body, offsets, counts = device_encode(dev, img, lay)
        raw = H.shim_gather(shim, img, lay)
        for o, c, r in zip(offsets, counts, raw):
            assert zlib.decompress(body[o:o + c]) == r
        huff = sum(len(H.huffman_only(r)) for r in raw)
        z1 = sum(len(zlib.compress(r, 1)) for r in raw)
        with capsys.disabled():
            print(f"\n{name}: device writer / zlib -1 = {len(body) / z1:.4f}, Huffman-only / zlib -1 = {huff / z1:.4f}")
        assert len(body) == sum(counts) < huff and len(body) / z1 <= recorded + 0.02


# ---------------------------------------------------------------- the C ABI on guarded buffers

def guarded_encode(dev, a, lay, fill, short_by=0, stream=None):
    """lbdrn_tiffw_encode on buffers of tests/guarded.py: (rc, body, offsets, counts, arena, the output buffers)"""
    import torch
    from lbdrn_hip import tiff_write
    L = tiff_write.lib()
    nseg = L.lbdrn_tiffw_segment_count(ctypes.byref(lay))
    nws, nout = L.lbdrn_tiffw_workspace(ctypes.byref(lay)), L.lbdrn_tiffw_output_bytes(ctypes.byref(lay))
    ar = Arena(dev)
    planes = ar.const(a, name="planes")
    out = ar.buf(nout, fill, name="out")
    offsets, counts, total = ar.buf(8 * nseg, fill, name="offsets"), ar.buf(8 * nseg, fill, name="counts"), ar.buf(8, fill, name="total")
    ws = ar.buf(nws - short_by, fill, name="workspace")
    rc = L.lbdrn_tiffw_encode(ctypes.byref(lay), planes.ptr, out.ptr, nout, offsets.ptr, counts.ptr, total.ptr, ws.ptr, nws - short_by,
                              None if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize(dev)
    if rc != 0:
        return rc, None, None, None, ar, (out, offsets, counts, total, ws)
    n = int(total.numpy(np.uint64)[0])
    assert n <= nout
    return rc, out.numpy(np.uint8)[:n].tobytes(), offsets.numpy(np.uint64).tolist(), counts.numpy(np.uint64).tolist(), ar, (out, offsets, counts, total, ws)


@pytest.mark.parametrize("compress", ("none", "deflate"))
def test_workspace_hygiene_and_determinism(dev, shim, compress):
    """fills 0x00 / 0xFF / 0xA5 of output, tables and workspace give the same bytes; the guards and the planes are intact; two
    runs and a run on another stream give the same bytes; a workspace one byte short is refused before a launch"""
    import torch
    from lbdrn_hip import tiff_write
    a = H.base_raster()[:4]
    for seg, planar in ((dict(tile=(16, 16)), 1), (dict(rows_per_strip=8), 2)):
        lay = tiff_write.make_layout(*a.shape, 16, compress, planar=planar, **seg)
        want = H.host_encode(shim, a, lay)
        want = (want[0].tobytes(), want[1].tolist(), want[2].tolist())
        for fill in FILLS:
            rc, body, offsets, counts, ar, _ = guarded_encode(dev, a, lay, fill)
            assert rc == 0, (tiff_write.lib().lbdrn_tiffw_last_error(), fill)
            ar.check()
            assert (body, offsets, counts) == want, (seg, fill)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            rc, body, offsets, counts, ar, _ = guarded_encode(dev, a, lay, 0xA5, stream=side)
        ar.check()
        assert rc == 0 and (body, offsets, counts) == want
        if compress == "deflate":
            rc, _, _, _, ar, bufs = guarded_encode(dev, a, lay, 0xA5, short_by=1)
            assert rc == tiff_write.E_WORKSPACE and b"workspace" in tiff_write.lib().lbdrn_tiffw_last_error()
            ar.check()
            for b in bufs:      # nothing was launched: every buffer still holds its fill
                assert bool((b.as_u8() == 0xA5).all()), b.name


# ---------------------------------------------------------------- the command line

def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f]


def _measures(path):
    return [r for r in _records(path) if r.startswith(("MSE", "PSNR", "Max error", "Total size"))]


@pytest.fixture(scope="module")
def streams(tmp_path_factory, dev):
    """two small .bin files (the shapes of tests/test_gpu_window_decode.py): one image, -sr 1; four tiles with a lossless
    residual layer, -sr 2"""
    import encode
    from lbdrn_hip.synth import synthetic_tile
    root = tmp_path_factory.mktemp("tiffw_cli")
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


@pytest.mark.parametrize("name", ("one", "layered"))
def test_decode_out_compress_gives_the_same_raster_and_records(dev, streams, name, tmp_path, monkeypatch):
    import decode
    from lbdrn_hip import raster_io, tiff
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    img, src, sub, bin_path = streams[name]
    recon, log = str(sub / f"{name}_recon.tif"), str(sub / "decode.txt")

    def whole(extra, org):
        for p in (recon, log):
            if os.path.exists(p):
                os.remove(p)
        assert decode.main(["-i", bin_path] + (["-org", src] if org else []) + extra) == 0
        return _measures(log) if org else open(recon, "rb").read()
    plain = whole([], False)
    rec = raster_io.read_raster(recon)
    ref = str(tmp_path / "ref.tif")
    raster_io._write_tiff(ref, rec)
    assert plain == open(ref, "rb").read()      # without the flag: the file the writer always wrote
    packed = whole(["--out-compress", "deflate", "--out-tile", "32"], False)
    lay = tiff.parse(packed).layout
    assert (lay.tiled, lay.seg_w, lay.seg_h, lay.compression, lay.predictor, lay.planar) == (1, 32, 32, 8, 2, 2)
    assert np.array_equal(raster_io.read_raster(recon), rec)
    if name == "layered":
        assert np.array_equal(rec, img)      # --max-error 0: the original, through the compressed file
    whole(["--out-compress", "deflate"], False)
    assert tiff.parse(open(recon, "rb").read()).layout.seg_w == 256 and np.array_equal(raster_io.read_raster(recon), rec)
    a, b = whole([], True), whole(["--out-compress", "deflate", "--out-tile", "16"], True)
    assert a == b and len(a) >= 3 and not os.path.exists(recon)
    # --window and -o
    x0, y0, w, h = 5, 7, 30, 21
    outs = []
    for extra in ([], ["--out-compress", "deflate", "--out-tile", "16"]):
        wlog, wout = str(sub / "decode_window.txt"), str(tmp_path / f"w{len(extra)}.tif")
        if os.path.exists(wlog):
            os.remove(wlog)
        assert decode.main(["-i", bin_path, "-org", src, "--window", str(x0), str(y0), str(w), str(h), "-o", wout] + extra) == 0
        outs.append((raster_io.read_raster(wout), _measures(wlog), open(wout, "rb").read()))
    assert np.array_equal(outs[0][0], rec[:, y0:y0 + h, x0:x0 + w]) and np.array_equal(outs[1][0], outs[0][0])
    assert outs[0][1] == outs[1][1] and len(outs[0][1]) >= 2
    assert outs[0][2][2] == 42 and tiff.parse(outs[1][2]).layout.compression == 8 and tiff.parse(outs[0][2]).layout.compression == 1
