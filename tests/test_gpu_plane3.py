"""LBB3, the MSB payload with inter-band prediction, on the GPU: the kernels of csrc/plane3.hip against the sequential
restatement tests/plane3_reference.py -- byte identity both ways and the round trip on the shared case list; LBB2's body from both libraries where the two formats coincide; repeatability;
guarded, pre-filled buffers; a capacity one byte short; the fixed list of damaged units; encode.py / decode.py under
LBDRN_BASE_CODEC=LBB3 against the default; and the sharded launch, sweep.py and LBDRN_REPORT_BOTH_BPSP under it."""
import contextlib
import ctypes
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plane3_reference as R  # noqa: E402
from guarded import Arena, FILLS, fill_id  # noqa: E402
from lbdrn_hip import container, ops, plane3  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = R.cases()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("name,x", CASES, ids=[n for n, _ in CASES])
def test_body_is_byte_identical_to_the_restatement_and_round_trips(dev, name, x):
    want = R.case_body(name, x)
    body = plane3.encode(ops.to_device_u16(x, dev))
    assert body == want, (len(body), len(want))
    C, H, W = x.shape
    assert plane3.info(body) == (C, H, W, R.WRITER_S)
    assert np.array_equal(ops.from_device_u16(plane3.decode(want, C, H, W, dev)), x)      # the GPU reads the restatement's bytes
    if x.size <= 40000:      # (the restatement's decoder is a Python loop per sample; the bytes are identical anyway)
        assert np.array_equal(R.decode(body), x)


@pytest.mark.parametrize("S", [64, 128, 512])
def test_reader_takes_other_unit_heights(dev, S):
    for name in ("3x257x65", "2x65x64", "16 bands"):
        x = dict(CASES)[name]
        body = R.case_body(name, x, S)
        assert plane3.info(body) == x.shape + (S,)
        assert np.array_equal(ops.from_device_u16(plane3.decode(body, *x.shape, dev)), x)


def _one_band_cases():
    """the smallest one-band shapes that reach the partial last strip (tw < 64), the short last pass (rows < 64), the carried row
    above (H > 64), the zero-group states (z0 = 2) and the 31-bit escape; H <= 256, the writer's S"""
    rng = np.random.default_rng(0)
    yield "one pixel", np.array([[[513]]], np.uint16)
    yield "one row", rng.integers(0, 300, (1, 1, 257)).astype(np.uint16)
    yield "one column", rng.integers(0, 300, (1, 130, 1)).astype(np.uint16)
    yield "constant", np.full((1, 65, 64), 40000, np.uint16)
    yield "noise 16 bit", rng.integers(0, 65536, (1, 129, 67)).astype(np.uint16)
    yield "sparse spikes", ((rng.random((1, 200, 130)) < 0.02) * rng.integers(0, 65536, (1, 200, 130))).astype(np.uint16)
    yield "zeros", np.zeros((1, 70, 90), np.uint16)


@pytest.mark.parametrize("name,x", list(_one_band_cases()), ids=[n for n, _ in _one_band_cases()])
def test_one_band_in_one_row_of_units_is_the_lbb2_body(dev, name, x):
    """The two libraries are built from one lane coder and one wave walk: where the formats coincide -- one band, no unit
    boundary inside the height -- liblbdrn_plane3.so writes liblbdrn_hip.so's LBB2 body behind its header, and reads it."""
    _, H, W = x.shape
    assert H <= R.WRITER_S
    x_d = ops.to_device_u16(x, dev)
    lbb2 = ops.plane_encode(x_d)
    assert plane3.encode(x_d)[4 * R.HEADER_WORDS:] == lbb2
    back = plane3.decode(R.MAGIC + struct.pack("<4I", 1, H, W, R.WRITER_S) + lbb2, 1, H, W, dev)      # (raises unless the status is 0)
    assert np.array_equal(ops.from_device_u16(back), x)


def test_two_encodes_give_the_same_bytes(dev):
    x = dict(CASES)["correlated_tile(1, 8, 300, 130) >> 5"]
    x_d = ops.to_device_u16(x, dev)
    assert plane3.encode(x_d) == plane3.encode(x_d)


def _gpu_encode(dev, A, x, fill, short=0):
    L = plane3.lib()
    C, H, W = x.shape
    planes = A.const(x, "planes")
    cap, nws = L.lbdrn_plane3_bound(C, H, W), L.lbdrn_plane3_encode_workspace(C, H, W)
    body, nbytes, ws = A.buf(cap, fill, name="body"), A.buf(8, fill, name="body_bytes"), A.buf(nws, fill, name="workspace")
    with torch.cuda.device(dev):
        rc = L.lbdrn_plane3_encode(planes.ptr, C, H, W, body.ptr, cap - short, nbytes.ptr, ws.ptr, nws, _stream(dev))
        torch.cuda.synchronize(dev)
    return rc, body, nbytes, ws


def _gpu_decode(dev, A, raw, geom, fill):
    L = plane3.lib()
    C, H, W, S = geom
    src = A.const(np.frombuffer(raw, np.uint8), "body")
    nws = L.lbdrn_plane3_decode_workspace(C, H, W)
    planes, status, ws = A.buf(2 * C * H * W, fill, name="planes"), A.buf(4, fill, name="status"), A.buf(nws, fill, name="workspace")
    with torch.cuda.device(dev):
        rc = L.lbdrn_plane3_decode(src.ptr, len(raw), C, H, W, S, planes.ptr, status.ptr, ws.ptr, nws, _stream(dev))
        torch.cuda.synchronize(dev)
    return rc, planes, status


@pytest.mark.parametrize("fill", FILLS, ids=[fill_id(f) for f in FILLS])
def test_guarded_prefilled_buffers_same_bytes_nothing_touched_outside(dev, fill):
    for name in ("3x257x65", "16 bands"):
        x = dict(CASES)[name]
        want = R.case_body(name, x)
        A = Arena(dev)
        rc, body, nbytes, _ = _gpu_encode(dev, A, x, fill)
        assert rc == 0, plane3.lib().lbdrn_plane3_last_error()
        n = int(nbytes.numpy(np.uint64)[0])
        assert n == len(want) and body.numpy(np.uint8, n).tobytes() == want
        assert (body.numpy(np.uint8)[n:] == fill).all()      # nothing behind the body's last byte either
        A.check()
        A = Arena(dev)
        rc, planes, status = _gpu_decode(dev, A, want, x.shape + (R.WRITER_S,), fill)
        assert rc == 0 and int(status.numpy(np.int32)[0]) == 0
        assert np.array_equal(planes.numpy(np.uint16).reshape(x.shape), x)
        A.check()


def test_capacity_one_byte_short_is_an_error_and_nothing_is_written(dev):
    x = dict(CASES)["2x65x64"]
    A = Arena(dev)
    rc, body, nbytes, ws = _gpu_encode(dev, A, x, 0xA5, short=1)
    assert rc == plane3.E_WORKSPACE and b"too small" in plane3.lib().lbdrn_plane3_last_error()
    for b in (body, nbytes, ws):
        assert (b.numpy(np.uint8) == 0xA5).all(), b.name
    A.check()
    with pytest.raises(ValueError, match="16"):
        container.encode_base(np.zeros((17, 4, 4), np.uint16), codec="LBB3")


def test_damaged_units_return_and_touch_nothing_outside(dev):
    """The fixed list tests/plane3_damage_main.cpp runs through the host decoder: every call returns; the body is refused on the
    host, flagged in *status, or decodes to merely wrong values; the guards around planes, status and workspace stay."""
    flagged = refused = passed = 0
    for name, raw, geom in R.damaged_units():
        A = Arena(dev)
        rc, planes, status = _gpu_decode(dev, A, raw, geom, 0xA5)
        A.check()
        if rc != 0:
            assert rc == plane3.E_ARG, (name, rc)
            assert (planes.numpy(np.uint8) == 0xA5).all(), name
            refused += 1
        elif int(status.numpy(np.int32)[0]):
            flagged += 1
        else:
            passed += 1
        if name == "sound":
            assert rc == 0 and passed == 1
        try:      # whatever the host validation refuses, the decoder flags or refuses too
            R.parse(raw)
        except R.Damaged:
            assert rc != 0 or int(status.numpy(np.int32)[0]), name
        if name in ("k0 = 16", "z0 = 3", "stray head bit", "band 0 differential", "mode bits beyond the bands", "unit 0: every taken word all ones",
                    "unit 0: every taken word zero", "header says S = 128", "stated as S = 128", "stated as 16 bands"):
            assert rc != 0 or int(status.numpy(np.int32)[0]), name
    assert flagged >= 15 and refused >= 2, (flagged, refused, passed)


def test_container_round_trip_and_keep_on_device(dev):
    x = dict(CASES)["correlated_tile(1, 8, 300, 130) >> 5"]
    for dtype in (np.uint16, np.uint8):
        msb = x.astype(dtype) if dtype == np.uint16 else (x >> 2).astype(np.uint8)
        payload = container.encode_base(msb, codec="LBB3")
        assert payload[:4] == b"LBB3" and payload[4] == (1 if dtype == np.uint8 else 2)
        assert payload == container.encode_base(ops.to_device_u16(msb.astype(np.uint16), dev), codec="LBB3", as_uint8=dtype == np.uint8)
        back = container.decode_base(payload)
        assert back.dtype == dtype and np.array_equal(back, msb)
        kept = container.decode_base(payload, keep_on_device=True)
        assert isinstance(kept, torch.Tensor) and kept.device.type == "cuda" and np.array_equal(ops.from_device_u16(kept), msb)
        assert len(payload) < 0.9 * len(container.encode_base(msb))      # the bands of this scene share their structure
    with pytest.raises(plane3.Plane3Error):
        container.decode_base(payload[:-4])


# ---------------------------------------------------------------- encode.py / decode.py

@contextlib.contextmanager
def _codec(name):
    import encode
    saved = encode.BASE_CODEC
    saved_env = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    try:
        encode.BASE_CODEC = name
        yield
    finally:
        encode.BASE_CODEC = saved
        for k, v in saved_env.items():
            if v is not None:
                os.environ[k] = v


def test_cli_under_lbb3_against_the_default(dev, tmp_path):
    import decode
    import encode
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import correlated_tile
    img = correlated_tile(3, 4, 48, 80)
    src = str(tmp_path / "scene.npy")
    np.save(src, img)
    out = {}
    for codec_name in ("LBB2", "LBB3"):
        work = tmp_path / codec_name
        with _codec(codec_name):
            assert encode.main(["-i", src, "-o", str(work), "-e", "1", "-bs", "512"]) == 0
            (sub,) = [d for d in work.iterdir() if d.is_dir()]
            binp = str(sub / "scene.bin")
            assert decode.main(["-i", binp]) == 0
            full = raster_io.read_raster(str(sub / "scene_recon.tif")).reshape(img.shape)
            wout = str(tmp_path / f"{codec_name}_window.tif")
            assert decode.main(["-i", binp, "--window", "10", "7", "33", "20", "-o", wout]) == 0
            window = raster_io.read_raster(wout).reshape(4, 20, 33)
            assert encode.main(["-i", src, "-o", str(work / "exact"), "-e", "1", "-bs", "512", "--max-error", "0"]) == 0
            (sub0,) = [d for d in (work / "exact").iterdir() if d.is_dir()]
            assert decode.main(["-i", str(sub0 / "scene.bin")]) == 0
            exact = raster_io.read_raster(str(sub0 / "scene_recon.tif")).reshape(img.shape)
        out[codec_name] = dict(raw=open(binp, "rb").read(), full=full, window=window, exact=exact)
    a, b = out["LBB2"], out["LBB3"]
    assert np.array_equal(a["full"], b["full"])                          # the rasters are equal bit for bit
    assert np.array_equal(b["window"], b["full"][:, 7:27, 10:43]) and np.array_equal(a["window"], b["window"])
    assert np.array_equal(b["exact"], img) and np.array_equal(a["exact"], img)
    assert np.array_equal(b["full"] >> 5, img >> 5)
    # the two files differ in the base payload and its length field, nowhere else
    ha, hb = container.unpack_header(a["raw"]), container.unpack_header(b["raw"])
    assert ha[:9] == hb[:9] and ha[9] != hb[9]
    n, nn = ha[0], ha[8][0]
    assert a["raw"][:n - 4] == b["raw"][:n - 4]                          # (one tile: the header ends with its base length)
    assert a["raw"][n:n + nn] == b["raw"][n:n + nn]
    pa, pb = a["raw"][n + nn:], b["raw"][n + nn:]
    assert len(pa) == ha[9][0] and len(pb) == hb[9][0] and pa[:4] == b"LBB2" and pb[:4] == b"LBB3"
    assert pa[4:15] == pb[4:15]
    assert np.array_equal(container.decode_base(pa), container.decode_base(pb))


def test_sharded_launch_sweep_and_report_both_under_lbb3(dev, tmp_path):
    """What lies downstream of the payload works unchanged: the four tiles of an image fitted by two torchrun ranks under
    LBDRN_BASE_CODEC=LBB3 give the single-process file byte for byte, every base payload in it is LBB3, the sharded decode
    reports its metrics, LBDRN_REPORT_BOTH_BPSP logs LBB2's size beside the one written, and sweep.py runs its points."""
    import re
    import subprocess
    import encode
    import sweep
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import correlated_tile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "lbdrn-msic_amd")
    img = correlated_tile(5, 4, 50, 62)
    src = tmp_path / "scene.tif"
    raster_io.write_raster(str(src), img)
    flags = ["-K", "4", "-D", "1", "-bs", "96", "-e", "2", "-sr", "2"]
    sub = "scene_r2_K4_bc64_nl2_D1_prec16_lr0.001_bs96_e2"
    saved_both = encode.REPORT_BOTH
    with _codec("LBB3"):
        try:
            encode.REPORT_BOTH = True
            assert encode.main(["-i", str(src), "-o", str(tmp_path / "one")] + flags, shard_tiles=False) == 0
        finally:
            encode.REPORT_BOTH = saved_both
        assert sweep.main(["--images", str(src), "--k", "3", "4", "-o", str(tmp_path / "sw"), "-D", "1", "-bs", "96", "-e", "1", "--summary"]) == 0
    one = (tmp_path / "one" / sub / "scene.bin").read_bytes()
    n, sr, _, _, _, _, _, _, nn, base = container.unpack_header(one)
    assert sr == 2 and len(base) == 4
    pos = n
    for a, b in zip(nn, base):
        assert one[pos + a:pos + a + 4] == b"LBB3"
        pos += a + b
    log = (tmp_path / "one" / sub / "encode.txt").read_text()
    both = re.findall(r"MSB as LBB2: (\d+) bytes.*\(written: LBB3\)", log)
    written = re.findall(r"MSB: (\d+) bytes", log)
    assert len(both) == 4 and len(written) == 4 and sum(map(int, written)) < sum(map(int, both))
    bins = [os.path.join(d, f) for d, _, files in os.walk(tmp_path / "sw") for f in files if f.endswith(".bin")]
    assert len(bins) == 2
    for path in bins:
        raw = open(path, "rb").read()
        h = container.unpack_header(raw)
        assert raw[h[0] + h[8][0]:h[0] + h[8][0] + 4] == b"LBB3"
    assert len([f for d, _, files in os.walk(tmp_path / "sw") for f in files if f.endswith(".csv")]) == 1
    # two ranks
    env = dict(os.environ, PYTHONPATH=pkg, HSA_ENABLE_IPC_MODE_LEGACY="0", LBDRN_BASE_CODEC="LBB3")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    run2 = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", str(29400 + os.getpid() % 200)]
    subprocess.run(run2 + [os.path.join(pkg, "encode.py"), "-i", str(src), "-o", str(tmp_path / "two")] + flags,
                   check=True, env=env, capture_output=True, timeout=300)
    assert (tmp_path / "two" / sub / "scene.bin").read_bytes() == one
    subprocess.run(run2 + [os.path.join(pkg, "decode.py"), "-i", str(tmp_path / "two" / sub / "scene.bin"), "-org", str(src)],
                   check=True, env=env, capture_output=True, timeout=300)
    assert "PSNR" in (tmp_path / "two" / sub / "decode.txt").read_text()      # (-org removes the raster behind the metrics)
    import decode
    with _codec("LBB2"):
        assert decode.main(["-i", str(tmp_path / "one" / sub / "scene.bin")], shard_tiles=False) == 0      # (the same bytes, not yet decoded)
    rec = raster_io.read_raster(str(tmp_path / "one" / sub / "scene_recon.tif")).reshape(img.shape)
    assert np.array_equal(rec >> 4, img >> 4)
