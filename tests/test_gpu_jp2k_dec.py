"""The GPU JPEG 2000 decoder (lbdrn_jp2kd_decode, csrc/jp2k_dec.hip; LBDRN_BASE_DECODER=gpu) on the device: round trips
through the public layer, files of foreign writers (a committed fixture of OpenJPEG files, the oracle's, OpenJPEG's and
Pillow's where present), the workspace contract on guarded buffers, refusals, damaged files, and the command line.  Every
comparison is exact.  On a mismatch the message names the first differing code block and says whether tier-1 (the slab
k_jp2k_unblocks left at the start of the workspace, which the inverse transform never writes, against
oracle.coefficients) or the inverse transform is at fault.  None of this needs OpenJPEG except the legs that say so."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import jp2k as oracle  # noqa: E402
from guarded import FILLS, Arena, fill_id  # noqa: E402
from test_gpu_jp2k import SYNTH  # noqa: E402
from test_jp2k_dec_host import GuardedBytes, check_damaged, corruptions, load_shim, small_files, truncations  # noqa: E402
from test_jp2k_oracle import NEW_GEOMETRY_PLANES, fuzz_planes, planes_of  # noqa: E402

pytestmark = pytest.mark.gpu
F = oracle.F


@pytest.fixture(autouse=True)
def gpu_reader(monkeypatch):
    monkeypatch.setenv("LBDRN_BASE_DECODER", "gpu")


def dec():
    from lbdrn_hip import jp2k_dec
    return jp2k_dec


def raw_decode(f, dev, ws=None, planes=None, ws_bytes=None):
    """lbdrn_jp2kd_decode through the test's own ctypes call -> (rc, message, planes tensor, workspace tensor, (C, H, W, bits))"""
    import torch
    d = dec()
    L = d.lib()
    C, H, W, bits = d.info(f)
    nws = L.lbdrn_jp2kd_workspace(f, len(f))
    assert nws > 0
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    if planes is None:
        planes = torch.empty((C, H, W), dtype=torch.int16, device=dev)
    rc = L.lbdrn_jp2kd_decode(f, len(f), ctypes.c_void_p(planes.data_ptr()), C, H, W, ctypes.c_void_p(ws.data_ptr()),
                              nws if ws_bytes is None else ws_bytes, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    return rc, (L.lbdrn_jp2kd_last_error() or b"").decode(errors="replace"), planes, ws, (C, H, W, bits)


def localise(f, x, dev):
    """Which stage is at fault when the file f does not decode to x: reads the coefficient slabs k_jp2k_unblocks left at the
    start of the workspace and compares them, block by block, with the oracle's coefficients of x (for a file of the
    encoder's own geometry) or with the oracle's tier-1 decoding of the file's blocks."""
    rc, msg, planes, ws, (C, H, W, bits) = raw_decode(f, dev)
    if rc:
        return f"lbdrn_jp2kd_decode answers {rc}: {msg}"
    i, rec = oracle.info(f), oracle.parse(f)
    tw, th = min(i["tw"], W), min(i["th"], H)
    slabs = ws[:i["tiles"] * C * tw * th * 4].cpu().numpy().view(np.int32).reshape(i["tiles"] * C, th, tw)
    own = oracle.layout(C, H, W, 16 if bits > 8 else 8)[2:5] == (i["tw"], i["th"], i["resolutions"]) and bits in (8, 16)
    coef = {}
    for r in rec:
        t, c, bx, by, bw, bh = (int(r[F[k]]) for k in ("tile", "comp", "x", "y", "w", "h"))
        got = slabs[t * C + c, by:by + bh, bx:bx + bw]
        if own:
            if (t, c) not in coef:
                coef[(t, c)] = oracle.coefficients(x, t, c)
            want = coef[(t, c)][by:by + bh, bx:bx + bw]
        elif r[F["passes"]]:
            data = f[r[F["offset"]]:r[F["offset"]] + r[F["length"]]]
            want = oracle.t1_decode(data, bw, bh, int(r[F["orient"]]), int(r[F["numbps"]]), int(r[F["passes"]]))
        else:
            want = np.zeros((bh, bw), np.int32)
        if not np.array_equal(got, want):
            where = ", ".join(f"{k} {int(r[F[k]])}" for k in ("tile", "comp", "res", "band", "gx", "gy"))
            return (f"first differing code block: {where} ({bw} x {bh}, orientation {int(r[F['orient']])}, numbps {int(r[F['numbps']])}, "
                    f"passes {int(r[F['passes']])}): {int((got != want).sum())} coefficients of the slab after k_jp2k_unblocks differ from "
                    f"the oracle's: TIER-1 (k_jp2k_unblocks / jp2k_t1d.inc / the block table) is at fault")
    return "every code block of the slab after k_jp2k_unblocks equals the oracle's: the INVERSE TRANSFORM (k_jp2k_unlift / k_jp2k_unshift) is at fault"


def assert_decodes_to(f, x, dev, label=""):
    """container.decode_base under LBDRN_BASE_DECODER=gpu gives x with its dtype"""
    from lbdrn_hip import container
    y = container.decode_base(f, device=dev)
    assert y.dtype == x.dtype and y.shape == x.shape, (label, y.dtype, y.shape, x.dtype, x.shape)
    if not np.array_equal(y, x):
        bad = np.argwhere(y != x)
        raise AssertionError(f"jp2k-dec {label} {x.shape} {x.dtype}: {len(bad)} samples differ, first at {tuple(bad[0])}; {localise(f, x, dev)}")
    return y


def assert_round_trip(x, dev, label=""):
    from lbdrn_hip import container
    f = container.encode_base(x, codec="jp2-gpu", device=dev)
    assert_decodes_to(f, x, dev, label)
    return f


# ------------------------------------------------------------------ round trips

@pytest.mark.parametrize("shape", SYNTH, ids=lambda s: "x".join(map(str, s)))
def test_synthetic_planes_round_trip(shape, dev):
    from lbdrn_hip.synth import synthetic_tile
    assert_round_trip(np.ascontiguousarray(synthetic_tile(0, *shape) >> 5), dev, "synthetic")


def test_eight_bit_empty_incompressible_and_spike_planes_round_trip_and_stay_on_the_device(dev):
    import torch
    from lbdrn_hip import container
    from lbdrn_hip.synth import synthetic_tile
    x8 = np.ascontiguousarray(synthetic_tile(0, 3, 300, 517) >> 8).astype(np.uint8)
    f = assert_round_trip(x8, dev, "8 bits")
    t = container.decode_base(f, device=dev, keep_on_device=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int16 and np.array_equal(t.cpu().numpy().view(np.uint16), x8)
    assert_round_trip(np.zeros((2, 100, 130), np.uint16), dev, "zero")
    assert_round_trip(np.full((2, 100, 130), 32768, np.uint16), dev, "zero after the level shift")
    assert_round_trip(np.full((3, 1100, 90), 1234, np.uint16), dev, "constant")
    assert_round_trip(np.full((1, 70, 70), 200, np.uint8), dev, "constant, 8 bits")
    x = np.random.default_rng(7).integers(0, 65536, (2, 257, 300)).astype(np.uint16)
    assert x.min() < 50 and x.max() > 65500
    f = assert_round_trip(x, dev, "uniform random")
    t = container.decode_base(f, device=dev, keep_on_device=True)
    assert t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint16), x)
    z = np.zeros((1, 130, 140), np.uint16)
    z[0, 77, 91] = 65535
    assert_round_trip(z, dev, "spike")
    z = np.zeros((2, 1030, 1100), np.uint16)
    z[1, 1029, 1099] = 65535
    assert_round_trip(z, dev, "spike in the last tile's corner")


@pytest.mark.parametrize("shape", NEW_GEOMETRY_PLANES, ids=lambda s: "x".join(map(str, s)))
def test_tile_edge_geometries_round_trip(shape, dev):
    assert_round_trip(planes_of("synth", shape, 16), dev, "geometry")
    if shape[1] * shape[2] < 400000:
        assert_round_trip(planes_of("uniform", shape, 8), dev, "geometry, 8 bits uniform")


def test_period_two_patterns_round_trip(dev):
    for shape in ((1, 300, 517), (2, 1030, 90), (1, 64, 64), (1, 7, 1100)):
        for stat in ("stripes_h", "stripes_v", "checker"):
            for bits in (16, 8):
                assert_round_trip(planes_of(stat, shape, bits), dev, stat)


def test_a_seeded_fuzz_of_shapes_depths_and_statistics_round_trips(dev):
    n = 0
    for shape, bits, stat, x in fuzz_planes(48, 20261016):
        assert_round_trip(x, dev, f"fuzz case {n} ({stat}, {bits} bits)")
        n += 1
    assert n == 48


# ------------------------------------------------------------------ foreign writers

def test_every_openjpeg_file_of_the_fixture_and_the_oracles_file_of_its_planes_decode(dev, golden):
    g = golden["jp2k_openjpeg"]
    names = sorted(k[len("file_"):] for k in g.files if k.startswith("file_"))
    assert len(names) >= 6
    for name in names:
        x = g["planes_" + name]
        assert_decodes_to(g["file_" + name].tobytes(), x, dev, f"fixture file {name}")
        assert_decodes_to(oracle.encode(x), x, dev, f"the oracle's file of {name}")


def test_files_openjpeg_writes_decode_and_equal_its_own_reading(dev):
    from lbdrn_hip import jp2
    if not jp2.available():
        pytest.skip("liblbdrn_jp2.so not built (OpenJPEG absent): this leg needs OpenJPEG to write the files")
    from lbdrn_hip.synth import synthetic_tile
    for shape, bits, stat in [((3, 300, 517), 16, "synth"), ((2, 1029, 1061), 16, "synth"), ((1, 33, 70), 8, "uniform"), ((2, 1, 200), 16, "synth"),
                              ((1, 1, 1), 16, "synth"), ((2, 100, 130), 16, "mid"), ((1, 130, 140), 16, "spike"), ((2, 90, 77), 8, "stripes_v")]:
        x = planes_of(stat, shape, bits)
        f = jp2.encode(x)
        y = assert_decodes_to(f, x, dev, f"OpenJPEG {stat}")
        assert np.array_equal(y, jp2.decode(f))
    x = np.ascontiguousarray(synthetic_tile(0, 8, 2048, 2048) >> 5)
    f = jp2.encode(x)
    assert np.array_equal(assert_decodes_to(f, x, dev, "OpenJPEG headline tile"), jp2.decode(f))


def test_reversible_files_pillow_writes_with_other_tiles_and_code_blocks_decode(dev):
    """What a file holds is what Pillow itself and the oracle read from it -- they must agree --, and that is what the
    decoder must return.  It is also the planes that were saved, except where Pillow's writer is at fault: this Pillow
    packs the samples of 16-bit TILED images wrongly (every tile but the first column's; OpenJPEG and the oracle read the
    same other samples from such a file), so for those two cases the file's content is the reference, not the input."""
    from PIL import Image, features
    if not features.check_codec("jpg_2000"):
        pytest.skip("this Pillow has no JPEG 2000 codec")
    n = faithful = 0
    for shape, bits, stat, kw in [((1, 300, 517), 16, "synth", dict(tile_size=(128, 96))), ((3, 300, 517), 8, "synth", dict(codeblock_size=(32, 32))),
                                  ((1, 333, 259), 8, "uniform", dict(tile_size=(100, 100), codeblock_size=(32, 32))),
                                  ((3, 200, 310), 8, "synth", dict(tile_size=(96, 70))),
                                  ((1, 90, 77), 16, "checker", dict(tile_size=(33, 45), num_resolutions=3)),
                                  ((1, 257, 300), 16, "synth", dict(num_resolutions=1)), ((1, 130, 140), 16, "sparse", dict(codeblock_size=(16, 64)))]:
        x = planes_of(stat, shape, bits)
        want = x[0] if shape[0] == 1 else x.transpose(1, 2, 0)
        buf = io.BytesIO()
        Image.fromarray(want).save(buf, "JPEG2000", irreversible=False, mct=0, **kw)
        f = buf.getvalue()
        im = Image.open(io.BytesIO(f))
        im.load()
        back = np.asarray(im).astype(x.dtype)
        held = np.ascontiguousarray(back[None] if shape[0] == 1 else back.transpose(2, 0, 1))
        assert np.array_equal(oracle.decode(f), held), (shape, kw)          # (the judge and the writer's own reader agree)
        if not (bits == 16 and "tile_size" in kw):
            assert np.array_equal(held, x), (shape, kw)
            faithful += 1
        assert_decodes_to(f, held, dev, f"Pillow {kw}")
        n += 1
    assert n == 7 and faithful == 5


# ------------------------------------------------------------------ stage localisation

def test_a_mismatch_names_the_block_and_the_stage(dev):
    """a file that is sound but decodes to OTHER planes than the ones claimed: a tier-1 difference (the first differing
    block is named), and planes that differ although every block agrees (the inverse transform is named)"""
    x = planes_of("synth", (2, 90, 130), 16)
    f = oracle.encode(x)
    assert "INVERSE TRANSFORM" in localise(f, x, dev)      # (nothing differs: every block of the slab equals the oracle's)
    y = x.copy()
    y[1, 40:50, 60:70] ^= 0x0100
    msg = localise(f, y, dev)
    assert "first differing code block: tile 0, comp 1" in msg and "TIER-1" in msg, msg
    with pytest.raises(AssertionError, match="first differing code block: tile 0, comp 1"):
        assert_decodes_to(f, y, dev, "wrong planes")


# ------------------------------------------------------------------ contract

@pytest.mark.parametrize("fill", FILLS, ids=fill_id)
def test_same_bits_from_poisoned_guarded_buffers(fill, dev):
    import torch
    L = dec().lib()
    cases = [planes_of("synth", (2, 300, 517), 16), planes_of("uniform", (3, 129, 200), 8), planes_of("sparse", (1, 1030, 70), 16),
             planes_of("mid", (2, 70, 90), 16)]
    for x in cases:
        f = oracle.encode(x)
        C, H, W = x.shape
        nws = L.lbdrn_jp2kd_workspace(f, len(f))
        arena = Arena(dev)
        ws = arena.buf(nws, fill, name="workspace")
        out = arena.buf(x.size * 2, fill, name="planes")
        rc = L.lbdrn_jp2kd_decode(f, len(f), out.ptr, C, H, W, ws.ptr, nws, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
        assert rc == 0, (L.lbdrn_jp2kd_last_error() or b"").decode()
        got = out.numpy(np.uint16).reshape(x.shape)
        assert np.array_equal(got, x.astype(np.uint16)), f"{x.shape} {fill_id(fill)}: {int((got != x).sum())} samples differ"
        arena.check()


def test_refusals_workspace_one_byte_short_wrong_geometry_and_unsupported_files(dev):
    import torch
    d = dec()
    L = d.lib()
    x = planes_of("synth", (2, 90, 130), 16)
    f = oracle.encode(x)
    nws = L.lbdrn_jp2kd_workspace(f, len(f))
    arena = Arena(dev)
    ws = arena.buf(nws, 0xA5, name="workspace")
    out = arena.buf(x.size * 2, 0xA5, name="planes")
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(data, C, H, W, ws_bytes):
        rc = L.lbdrn_jp2kd_decode(data, len(data), out.ptr, C, H, W, ws.ptr, ws_bytes, stream)
        torch.cuda.synchronize(dev)
        return rc, (L.lbdrn_jp2kd_last_error() or b"").decode()
    rc, msg = call(f, 2, 90, 130, nws - 1)
    assert rc == d.E_WORKSPACE and "workspace" in msg and str(nws) in msg
    rc, msg = call(f, 2, 90, 131, nws)
    assert rc == d.E_ARG and "2 x 90 x 130" in msg
    cod = f.index(b"\xff\x52", f.index(b"jp2c"))
    for pos, value, word in ((cod + 13, 0, "9/7"), (cod + 7, 2, "layers"), (cod + 12, 1, "style"), (cod + 4, 1, "precinct")):
        bad = bytearray(f)
        bad[pos] = value
        rc, msg = call(bytes(bad), 2, 90, 130, nws)
        assert rc == d.E_UNSUPPORTED and word in msg, (word, rc, msg)
    # nothing was launched or written by any refusal
    assert bool((out.as_u8() == 0xA5).all()) and bool((ws.as_u8() == 0xA5).all())
    arena.check()
    rc, msg = call(f, 2, 90, 130, nws)
    assert rc == 0 and np.array_equal(out.numpy(np.uint16).reshape(x.shape), x)
    arena.check()
    # the public layer: an unsupported file raises with the library's message where OpenJPEG cannot take over
    from lbdrn_hip import container, jp2
    bad = bytearray(f)
    bad[cod + 7] = 2
    if not jp2.available():
        with pytest.raises(d.Jp2kDecUnsupported, match="layers"):
            container.decode_base(bytes(bad), device=dev)


def test_damaged_files_give_an_error_or_a_raster_with_the_guards_intact(dev, golden, tmp_path_factory):
    """Truncated and corrupted files -- each one first through the CPU build of the same parser (behind a guard page),
    then once through the device: an error, or a raster of some values; never a write outside the buffers."""
    import torch
    d = dec()
    L = d.lib()
    shim = load_shim(tmp_path_factory)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ran = refused = 0
    for name, f in small_files(golden):
        C, H, W, bits = d.info(f)
        room = GuardedBytes(len(f))
        nws = L.lbdrn_jp2kd_workspace(f, len(f))
        damaged = truncations(f, 200)[::17] + corruptions(f, 500)[::13]
        # corruptions of block data too: the block decoder runs on bytes that are not what its coder wrote
        rng = np.random.default_rng(3)
        for k in range(12):
            b = bytearray(f)
            for pos in rng.integers(len(f) // 2, len(f) - 2, 1 + k % 4):
                b[int(pos)] = int(rng.integers(256))
            damaged.append(bytes(b))
        for k, data in enumerate(damaged):
            table = check_damaged(shim, f"{name} damaged {k}", data, room)          # the CPU build first
            try:
                geometry = d.info(data)
            except d.Jp2kDecError:
                refused += 1
                continue
            assert table is not None
            c2, h2, w2, _ = geometry
            need = L.lbdrn_jp2kd_workspace(data, len(data))
            if c2 * h2 * w2 > 1 << 24 or need > 1 << 28:      # (a corrupted size field: not worth the memory)
                continue
            arena = Arena(dev)
            ws = arena.buf(need, 0xA5, name="workspace")
            out = arena.buf(c2 * h2 * w2 * 2, 0xA5, name="planes")
            rc = L.lbdrn_jp2kd_decode(data, len(data), out.ptr, c2, h2, w2, ws.ptr, need, stream)
            torch.cuda.synchronize(dev)
            assert rc in (0, d.E_ARG, d.E_UNSUPPORTED), (name, k, rc)
            arena.check()
            ran += 1
    print(f"damaged files: {refused} refused on the host, {ran} decoded on the device")
    assert ran > 0 and refused > 0


# ------------------------------------------------------------------ command line

def _cli_files(tmp_path, dev):
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import synthetic_tile
    img = synthetic_tile(21, 4, 80, 112)
    src = tmp_path / "tile.tif"
    raster_io.write_raster(str(src), img)
    name = "tile_r2_K5_bc64_nl2_D2_prec16_lr0.001_bs256_e2"
    bins = {}
    for codec_name in ("jp2-gpu", "LBB2"):
        env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lbdrn-msic_amd"), LBDRN_BASE_CODEC=codec_name)
        env.pop("LBDRN_BASE_DECODER", None)
        out = tmp_path / codec_name
        subprocess.run([sys.executable, os.path.join(ROOT, "lbdrn-msic_amd", "encode.py"), "-i", str(src), "-o", str(out),
                        "-K", "5", "-D", "2", "-bs", "256", "-e", "2", "-sr", "2"], check=True, env=env, capture_output=True)
        bins[codec_name] = out / name / "tile.bin"
    return img, bins


def _cli_decode(path, env_extra, out_name):
    """decode.py in a process of its own (the readers read their environment when they are imported)"""
    from lbdrn_hip import raster_io
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "lbdrn-msic_amd"))
    env.pop("LBDRN_BASE_DECODER", None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "lbdrn-msic_amd", "decode.py"), "-i", str(path)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    recon = path.parent / "tile_recon.tif"
    x = raster_io.read_raster(str(recon))
    os.replace(recon, path.parent / out_name)
    return x


def test_cli_round_trip_with_the_gpu_decoder_equals_the_lbb2_round_trip(dev, tmp_path):
    img, bins = _cli_files(tmp_path, dev)
    lbb2 = _cli_decode(bins["LBB2"], {}, "lbb2.tif")
    gpu = _cli_decode(bins["jp2-gpu"], {"LBDRN_BASE_DECODER": "gpu"}, "gpu.tif")
    assert np.array_equal(gpu, lbb2) and np.array_equal(gpu >> 5, img >> 5)


def test_a_jp2_gpu_file_decodes_where_openjpeg_is_not_built(dev, tmp_path):
    """LBDRN_JP2_LIB names a missing file -- a box without OpenJPEG -- and LBDRN_BASE_DECODER is unset: the default reader
    takes the GPU decoder there, where the .bin could not be read before (Jp2Error)."""
    img, bins = _cli_files(tmp_path, dev)
    lbb2 = _cli_decode(bins["LBB2"], {}, "lbb2.tif")
    alone = _cli_decode(bins["jp2-gpu"], {"LBDRN_JP2_LIB": str(tmp_path / "no_such_liblbdrn_jp2.so")}, "alone.tif")
    assert np.array_equal(alone, lbb2) and np.array_equal(alone >> 5, img >> 5)
