"""The GPU JPEG 2000 encoder (base codec "jp2-gpu": lbdrn_jp2k_encode, csrc/jp2k.hip) judged twice.  By the oracle
(oracle/jp2k_oracle.c, proven on the CPU by tests/test_jp2k_oracle.py): its files equal the oracle's byte for byte, and a
mismatch names the first differing code block and the stage at fault; these tests need no OpenJPEG.  And by OpenJPEG,
where liblbdrn_jp2.so is built: the files decode to exactly the planes that went in, carry the marker segments of the host
codec's files (lbdrn_hip/jp2.py, csrc/jp2_shim.c), and have their size up to the arithmetic coder's termination."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import jp2k as oracle  # noqa: E402
from test_jp2k_oracle import NEW_GEOMETRY_PLANES, fuzz_planes, planes_of  # noqa: E402

pytestmark = pytest.mark.gpu

SYNTH = [(8, 2048, 2048), (4, 1029, 1061), (3, 300, 517), (1, 33, 70), (5, 1025, 64), (2, 1, 200), (1, 1, 1)]


@pytest.fixture(scope="module")
def jp2():
    from lbdrn_hip import jp2 as mod
    if not mod.available():
        pytest.skip("liblbdrn_jp2.so not built (OpenJPEG absent): no decoder to judge the stream")
    return mod


def gpu_encode(x, dev):
    """numpy planes -> .jp2 bytes through the public layer (container.encode_base, codec jp2-gpu)"""
    from lbdrn_hip import container
    return container.encode_base(x, codec="jp2-gpu", device=dev)


def segments(buf):
    """{marker: bytes of the main header's marker segment}, the offsets and lengths of the tile-parts (walked by Psot,
    never searched for in coded data), and the offset of the first SOT"""
    buf = bytes(buf)
    at = buf.index(b"jp2c") + 4
    assert buf[at:at + 2] == b"\xff\x4f"
    at += 2
    segs = {}
    while buf[at:at + 2] != b"\xff\x90":
        n = int.from_bytes(buf[at + 2:at + 4], "big")
        segs[buf[at:at + 2]] = buf[at:at + 2 + n]
        at += 2 + n
    first, parts = at, []
    while buf[at:at + 2] == b"\xff\x90":
        psot = int.from_bytes(buf[at + 6:at + 10], "big")
        parts.append((at, psot))
        at += psot
    assert buf[at:] == b"\xff\xd9"
    return segs, parts, first


def check_against_host_codec(x, dev, jp2):
    """lossless through OpenJPEG, same SIZ / COD / QCD and tile-part count as jp2.encode(x), size within
    4 bytes per code block + 64 of it; returns (gpu file, host file)"""
    from lbdrn_hip import _lib
    g = gpu_encode(x, dev)
    assert g[:12] == jp2.SIGNATURE
    y = jp2.decode(g)
    assert y.dtype == x.dtype and y.shape == x.shape and np.array_equal(y, x), (x.shape, int((y != x).sum()))
    h = jp2.encode(x)
    sg, pg, fg = segments(g)
    sh, ph, fh = segments(h)
    for marker in (b"\xff\x51", b"\xff\x52", b"\xff\x5c"):
        assert sg[marker] == sh[marker], (x.shape, marker.hex(), sg[marker].hex(), sh[marker].hex())
    assert len(pg) == len(ph)
    assert g[:g.index(b"jp2c") - 4] == h[:h.index(b"jp2c") - 4]     # the boxes in front of the codestream, byte for byte
    C, H, W = x.shape
    nblk = _lib.lib().lbdrn_jp2k_block_count(C, H, W)
    com = len(sh.get(b"\xff\x64", b"")) - len(sg.get(b"\xff\x64", b""))
    print(f"jp2-gpu {x.shape} {x.dtype}: {len(g)} bytes, OpenJPEG {len(h)} (its COM segment: {com}), {nblk} blocks, "
          f"tile-part data identical: {g[fg:] == h[fh:]}")
    assert len(h) - 4 * nblk - 64 <= len(g) <= len(h) + 4 * nblk + 64, (len(g), len(h), nblk)
    assert len(g) <= _lib.lib().lbdrn_jp2k_bound(C, H, W)
    return g, h


@pytest.mark.parametrize("shape", SYNTH, ids=lambda s: "x".join(map(str, s)))
def test_synthetic_planes_are_lossless_and_structured_like_the_host_codec(shape, dev, jp2):
    from lbdrn_hip.synth import synthetic_tile
    x = np.ascontiguousarray(synthetic_tile(0, *shape) >> 5)
    assert x.dtype == np.uint16
    g, h = check_against_host_codec(x, dev, jp2)
    siz = segments(g)[0][b"\xff\x51"]
    assert siz[40] == 15 and len(siz) == 40 + 3 * shape[0]      # Ssiz: 16 bits unsigned


def test_eight_bit_planes_get_precision_eight(dev, jp2):
    from lbdrn_hip.synth import synthetic_tile
    x = np.ascontiguousarray(synthetic_tile(0, 3, 300, 517) >> 8)
    assert x.max() <= 255
    g, _ = check_against_host_codec(x.astype(np.uint8), dev, jp2)
    segs = segments(g)[0]
    assert segs[b"\xff\x51"][40] == 7 and segs[b"\xff\x5c"][4:9] == bytes([0x40, 0x40, 0x48, 0x48, 0x50])


def test_empty_blocks_incompressible_planes_and_a_lone_spike(dev, jp2):
    """all-zero and constant planes (after the level shift: one value everywhere, high-pass blocks without a pass);
    uniform random planes over the whole 16-bit range (the stream is larger than the planes and must fit the bound); one
    sample of 65535 in a plane of zeros"""
    check_against_host_codec(np.zeros((2, 100, 130), np.uint16), dev, jp2)
    check_against_host_codec(np.full((2, 100, 130), 32768, np.uint16), dev, jp2)     # zero after the level shift: no pass at all
    check_against_host_codec(np.full((3, 1100, 90), 1234, np.uint16), dev, jp2)
    check_against_host_codec(np.full((1, 70, 70), 200, np.uint8), dev, jp2)
    x = np.random.default_rng(7).integers(0, 65536, (2, 257, 300)).astype(np.uint16)
    assert x.min() < 50 and x.max() > 65500
    g, _ = check_against_host_codec(x, dev, jp2)
    assert len(g) > x.nbytes
    z = np.zeros((1, 130, 140), np.uint16)
    z[0, 77, 91] = 65535
    check_against_host_codec(z, dev, jp2)
    z = np.zeros((2, 1030, 1100), np.uint16)
    z[1, 1029, 1099] = 65535
    check_against_host_codec(z, dev, jp2)


def test_pillow_reads_it_too(dev, jp2):
    from PIL import Image, features
    if not features.check_codec("jpg_2000"):
        pytest.skip("this Pillow has no JPEG 2000 codec")
    from lbdrn_hip.synth import synthetic_tile
    x = np.ascontiguousarray(synthetic_tile(0, 1, 300, 517) >> 5)
    im = Image.open(io.BytesIO(gpu_encode(x, dev)))
    im.load()
    assert np.array_equal(np.asarray(im).astype(np.uint16), x[0])
    rgb = np.ascontiguousarray((synthetic_tile(0, 3, 300, 517) >> 8).astype(np.uint8))
    im = Image.open(io.BytesIO(gpu_encode(rgb, dev)))
    im.load()
    assert np.array_equal(np.asarray(im), rgb.transpose(1, 2, 0))


def test_deterministic_alone_and_beside_a_fit(dev, jp2):
    import torch
    from lbdrn_hip import codec, ops
    from lbdrn_hip.features import FeatCfg
    from lbdrn_hip.synth import synthetic_tile
    x = np.ascontiguousarray(synthetic_tile(3, 4, 700, 1100) >> 5)
    planes = ops.to_device_u16(x, dev)
    a = ops.jp2k_encode(planes, 16)
    b = ops.jp2k_encode(planes, 16)
    assert a == b and np.array_equal(jp2.decode(a), x)
    # another tile's fit in flight on the default stream, the encoder on a stream of its own
    other = ops.to_device_u16(synthetic_tile(5, 8, 256, 256), dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.manual_seed(19920517)
    fit = codec.fit_device(other, 5, 2, 64, 2, 1e-3, 512, 3, cfg=FeatCfg())     # asynchronous launches
    with torch.cuda.stream(side):
        c = ops.jp2k_encode(planes, 16)
    torch.cuda.synchronize(dev)
    assert c == a
    assert fit.best_params is not None


def test_refusals_write_nothing_beyond_the_capacity(dev, jp2):
    import torch
    from lbdrn_hip import _lib, ops
    L = _lib.lib()
    x = (np.arange(2 * 90 * 120, dtype=np.uint16).reshape(2, 90, 120) * 7) % 251
    planes = ops.to_device_u16(x, dev)
    good = ops.jp2k_encode(planes, 8)
    assert np.array_equal(jp2.decode(good), x.astype(np.uint8))
    ws = torch.empty(L.lbdrn_jp2k_workspace(2, 90, 120), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(t, C, H, W, bits, cap, ws_bytes=None):
        buf = np.full(cap + 64, 0xA5, np.uint8)
        n = ctypes.c_size_t(12345)
        rc = L.lbdrn_jp2k_encode(ctypes.c_void_p(t.data_ptr()), C, H, W, bits, buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n),
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel() if ws_bytes is None else ws_bytes, stream)
        assert (buf[cap:] == 0xA5).all(), "bytes beyond the capacity were written"
        return rc, buf[:cap], n.value, (L.lbdrn_last_error() or b"").decode()

    rc, buf, n, _ = call(planes, 2, 90, 120, 8, len(good))                 # exactly enough
    assert rc == 0 and n == len(good) and buf.tobytes() == good
    rc, buf, n, msg = call(planes, 2, 90, 120, 8, len(good) - 1)           # one byte short
    assert rc == _lib.E_WORKSPACE and str(len(good)) in msg and n == 0 and (buf == 0xA5).all()
    big = x.copy()
    big[1, 50, 60] = 256
    rc, buf, n, msg = call(ops.to_device_u16(big, dev), 2, 90, 120, 8, len(good) + 100)
    assert rc == _lib.E_ARG and "8 bits" in msg and n == 0 and (buf == 0xA5).all()
    rc, _, _, msg = call(planes, 0, 90, 120, 8, 4096)
    assert rc == _lib.E_ARG and msg
    rc, _, _, msg = call(planes, 2, 90, 120, 12, 4096)
    assert rc == _lib.E_ARG and "bits" in msg
    rc, _, _, msg = call(planes, 2, 90, 120, 8, len(good), ws_bytes=1000)
    assert rc == _lib.E_WORKSPACE and "workspace" in msg


def test_cli_round_trip_with_the_gpu_jpeg2000_payload(dev, jp2, tmp_path):
    """LBDRN_BASE_CODEC=jp2-gpu, four tiles: every MSB payload in the .bin is a JP2 file, decode.py reconstructs what it
    reconstructs from the default (LBB2) file bit for bit, and LBDRN_REPORT_BOTH_BPSP still reports the other format."""
    from lbdrn_hip import container, raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(21, 4, 80, 112)
    src = tmp_path / "tile.tif"
    raster_io.write_raster(str(src), img)
    recs = {}
    name = "tile_r2_K5_bc64_nl2_D2_prec16_lr0.001_bs256_e2"
    for codec_name in ("jp2-gpu", "LBB2"):
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lbdrn-msic_amd"), LBDRN_BASE_CODEC=codec_name, LBDRN_REPORT_BOTH_BPSP="1")
        out = tmp_path / codec_name
        subprocess.run([sys.executable, os.path.join(ROOT, "lbdrn-msic_amd", "encode.py"), "-i", str(src), "-o", str(out),
                        "-K", "5", "-D", "2", "-bs", "256", "-e", "2", "-sr", "2"], check=True, env=env, capture_output=True)
        raw = (out / name / "tile.bin").read_bytes()
        n, sr, w, h, K, bc, nl, D, nn, base = container.unpack_header(raw)
        assert sr == 2 and len(base) == 4
        pos = n
        for t in range(4):
            payload = raw[pos + nn[t]:pos + nn[t] + base[t]]
            pos += nn[t] + base[t]
            assert (payload[:12] == jp2.SIGNATURE) == (codec_name == "jp2-gpu")
            msb = container.decode_base(payload)
            i, j = divmod(t, 2)
            assert np.array_equal(msb, img[:, 40 * i:40 * i + 40, 56 * j:56 * j + 56] >> 5)
        assert pos == len(raw)
        import decode as dec_mod
        sys.argv = ["decode.py"]
        assert dec_mod.main(["-i", str(out / name / "tile.bin")]) == 0
        recs[codec_name] = raster_io.read_raster(str(out / name / "tile_recon.tif"))
        logs = "".join(p.read_text() for p in sorted((out / name).glob("*.txt")))
        assert "coded beside the fit" not in logs
        other = re.search(r"MSB as (jp2|LBB2): (\d+) bytes: bpsp=", logs)
        assert other and other.group(1) == ("LBB2" if codec_name == "jp2-gpu" else "jp2")
    assert np.array_equal(recs["jp2-gpu"], recs["LBB2"]) and np.array_equal(recs["jp2-gpu"] >> 5, img >> 5)


# ------------------------------------------------------------------ the device against the oracle, byte for byte

def assert_equals_oracle(x, dev, label=""):
    """the device's file of x equals the oracle's; otherwise the message names the first differing code block, what
    differs in it, and whether the block coder or the transform / staging is at fault.  Returns the file."""
    g = gpu_encode(x, dev)
    o = oracle.encode(x)
    assert g == o, f"jp2-gpu {label} {x.shape} {x.dtype}: {oracle.first_difference(g, o, x)}"
    return g


@pytest.mark.parametrize("shape", SYNTH, ids=lambda s: "x".join(map(str, s)))
def test_synthetic_planes_equal_the_oracle_byte_for_byte(shape, dev):
    from lbdrn_hip.synth import synthetic_tile
    assert_equals_oracle(np.ascontiguousarray(synthetic_tile(0, *shape) >> 5), dev, "synthetic")


def test_eight_bit_empty_incompressible_and_spike_planes_equal_the_oracle(dev):
    from lbdrn_hip.synth import synthetic_tile
    assert_equals_oracle(np.ascontiguousarray(synthetic_tile(0, 3, 300, 517) >> 8).astype(np.uint8), dev, "8 bits")
    assert_equals_oracle(np.zeros((2, 100, 130), np.uint16), dev, "zero")
    assert_equals_oracle(np.full((2, 100, 130), 32768, np.uint16), dev, "zero after the level shift")
    assert_equals_oracle(np.full((3, 1100, 90), 1234, np.uint16), dev, "constant")
    assert_equals_oracle(np.full((1, 70, 70), 200, np.uint8), dev, "constant, 8 bits")
    assert_equals_oracle(np.random.default_rng(7).integers(0, 65536, (2, 257, 300)).astype(np.uint16), dev, "uniform random")
    z = np.zeros((1, 130, 140), np.uint16)
    z[0, 77, 91] = 65535
    assert_equals_oracle(z, dev, "spike")
    z = np.zeros((2, 1030, 1100), np.uint16)
    z[1, 1029, 1099] = 65535
    assert_equals_oracle(z, dev, "spike in the last tile's corner")


@pytest.mark.parametrize("shape", NEW_GEOMETRY_PLANES, ids=lambda s: "x".join(map(str, s)))
def test_tile_edge_geometries_equal_the_oracle(shape, dev):
    """sides of exactly 1024 and of 1025, one-pixel-wide last tiles, H = 1 tiled, ragged last tiles, 32768 on a side"""
    assert_equals_oracle(planes_of("synth", shape, 16), dev, "geometry")
    if shape[1] * shape[2] < 400000:
        assert_equals_oracle(planes_of("uniform", shape, 8), dev, "geometry, 8 bits uniform")


def test_period_two_patterns_keep_every_block_within_its_bands_bit_planes(dev):
    """stripes and checkerboards of 0 / 65535 (0 / 255) maximise the high-pass magnitudes; a block with more bit-planes than
    its band announces would get a negative zero-bit-plane count, which put_packet_header writes without complaint"""
    F = oracle.F
    for shape in ((1, 300, 517), (2, 1030, 90), (1, 64, 64), (1, 7, 1100)):
        for stat in ("stripes_h", "stripes_v", "checker"):
            for bits in (16, 8):
                g = assert_equals_oracle(planes_of(stat, shape, bits), dev, stat)
                rec = oracle.parse(g)
                assert (rec[:, F["numbps"]] <= rec[:, F["mb"]]).all(), (shape, stat, bits, rec[rec[:, F["numbps"]] > rec[:, F["mb"]]][:3])
                assert rec[:, F["numbps"]].max() >= bits, (shape, stat, bits)      # (the patterns do reach the high planes)


def test_a_seeded_fuzz_of_shapes_depths_and_statistics_equals_the_oracle(dev):
    n = 0
    for shape, bits, stat, x in fuzz_planes(48, 20261016):
        assert_equals_oracle(x, dev, f"fuzz case {n} ({stat}, {bits} bits)")
        n += 1
    assert n == 48


@pytest.mark.parametrize("side", [6000, 7550])
def test_one_component_of_a_scene_equals_the_oracle(side, dev):
    """The two scene sizes of README.md, one component each (36 and 57 million samples in 36 and 64 tiles).  The oracle's
    coding time decides how much of a scene is affordable: one core codes 1 x 6000 x 6000 in 7.6 s and
    1 x 7550 x 7550 in 11.2 s (plus 4 s and 6 s to make the planes), so all eight (four) components would cost over a minute of a shared machine's
    time per run; the geometry is the same for every component, one is coded."""
    from lbdrn_hip.synth import synthetic_tile
    assert_equals_oracle(np.ascontiguousarray(synthetic_tile(0, 1, side, side) >> 5), dev, "scene")


def test_poisoned_workspace_changes_nothing_and_the_guard_behind_it_stays(dev):
    """The caller's workspace holds whatever the last user left: the file from a workspace pre-filled with 0xA5 equals the
    one from a zeroed workspace, and nothing is written behind lbdrn_jp2k_workspace bytes (a guard region in the same
    tensor, memory this test owns).  16 bits, 8 bits (whose carve differs from the 16-bit sizing), and a small sparse
    image coded straight after a large dense one in the same workspace."""
    import torch
    from lbdrn_hip import _lib, ops
    L = _lib.lib()
    GUARD = 1 << 16
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(planes, x, bits, ws, ws_bytes):
        C, H, W = x.shape
        cap = L.lbdrn_jp2k_bound(C, H, W)
        buf = np.zeros(cap, np.uint8)
        n = ctypes.c_size_t(0)
        rc = L.lbdrn_jp2k_encode(ctypes.c_void_p(planes.data_ptr()), C, H, W, bits, buf.ctypes.data_as(ctypes.c_void_p), cap,
                                 ctypes.byref(n), ctypes.c_void_p(ws.data_ptr()), ws_bytes, stream)
        assert rc == 0, (L.lbdrn_last_error() or b"").decode()
        torch.cuda.synchronize(dev)
        return buf[:n.value].tobytes()

    dense = np.random.default_rng(11).integers(0, 65536, (2, 1030, 300)).astype(np.uint16)
    sparse = planes_of("sparse", (1, 70, 90), 16)
    eight = planes_of("uniform", (3, 129, 200), 8)
    for x in (dense, eight, planes_of("synth", (2, 300, 517), 16)):
        bits = 8 * x.dtype.itemsize
        planes = ops.to_device_u16(x.astype(np.uint16), dev)
        nws = L.lbdrn_jp2k_workspace(*x.shape)
        ws = torch.empty(nws + GUARD, dtype=torch.uint8, device=dev)
        ws.zero_()
        ws[nws:] = 0xA5
        clean = call(planes, x, bits, ws, nws)
        ws.fill_(0xA5)
        dirty = call(planes, x, bits, ws, nws)
        assert dirty == clean, f"{x.shape} {bits} bits: {oracle.first_difference(dirty, clean, x)}"
        assert clean == oracle.encode(x), oracle.first_difference(clean, oracle.encode(x), x)
        assert bool((ws[nws:] == 0xA5).all()), f"{x.shape} {bits} bits: bytes behind the workspace were written"
    # the small sparse image straight after the large dense one, in the workspace the dense one left behind
    nws = L.lbdrn_jp2k_workspace(*dense.shape)
    ws = torch.empty(nws + GUARD, dtype=torch.uint8, device=dev)
    ws.fill_(0xA5)
    assert call(ops.to_device_u16(dense, dev), dense, 16, ws, nws) == oracle.encode(dense)
    small = L.lbdrn_jp2k_workspace(*sparse.shape)
    assert small < nws
    got = call(ops.to_device_u16(sparse, dev), sparse, 16, ws, nws)
    assert got == oracle.encode(sparse), oracle.first_difference(got, oracle.encode(sparse), sparse)
    assert bool((ws[nws:] == 0xA5).all()), "bytes behind the workspace were written"
