"""codec.decode_window / decode.py --window on the GPU: every window equals the same crop of the whole reconstruction bit for
bit -- for each shape, kernel path, MSB payload codec and activation a file may carry --, tiles the window does not touch
are not read, and the normaliser is the whole tile's MSB maximum.

Every case is encoded once per module (encode.main, one epoch: the fit's quality is irrelevant) and decoded whole once
(decode.main); the windows are compared against that raster."""
import contextlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _settings(consts=None, base_codec=None, env=None):
    """constants.py switches (not stored in the file: both sides must agree), encode.py's payload codec, environment."""
    import constants
    import encode
    saved_c = {k: getattr(constants, k) for k in (consts or {})}
    saved_codec = encode.BASE_CODEC
    saved_env = {k: os.environ.get(k) for k in list(env or {}) + ["RANK", "WORLD_SIZE", "LOCAL_RANK"]}
    try:
        for k, v in (consts or {}).items():
            setattr(constants, k, v)
        if base_codec is not None:
            encode.BASE_CODEC = base_codec
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)
        os.environ.update(env or {})
        yield
    finally:
        for k, v in saved_c.items():
            setattr(constants, k, v)
        encode.BASE_CODEC = saved_codec
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _spike(img):
    """The tile's MSB maximum in one pixel of the last row, far above the rest: a window elsewhere has another maximum."""
    img = (img >> 3).astype(np.uint16)
    img[:, -1, -1] = 60000
    return img


# name -> (C, H, W), encode flags, constants, payload codec, environment while decoding, image hook
CASES = {
    "headline": ((8, 40, 52), ["-K", "5", "-D", "2", "-bc", "64", "-nl", "2", "-sr", "1"], {}, None, {}, None),
    "ragged": ((4, 50, 37), ["-D", "1", "-sr", "2"], {}, None, {}, None),
    "nine": ((8, 48, 48), ["-D", "3", "-sr", "3"], {}, None, {}, None),
    "generic": ((3, 33, 21), ["-D", "0", "-bc", "32", "-nl", "1"], {}, None, {}, None),
    "embed": ((8, 24, 20), ["-D", "2"], {"USE_COORDINATES": True, "EMBEDDING": True}, None, {}, None),
    "coords": ((4, 26, 30), ["-D", "1", "-sr", "2"], {"USE_COORDINATES": True, "EMBEDDING": False}, None, {}, None),
    "relu": ((4, 30, 26), ["-D", "2", "-sr", "2"], {"HIDDEN_ACTIVATION": "relu"}, None, {}, None),
    "wide": ((4, 32, 36), ["-D", "2", "-bc", "256"], {}, None, {}, None),
    "jp2gpu": ((4, 50, 37), ["-D", "2", "-sr", "2"], {}, "jp2-gpu", {"LBDRN_BASE_DECODER": "gpu"}, None),
    "jp2": ((4, 50, 37), ["-D", "2", "-sr", "2"], {}, "jp2", {"LBDRN_BASE_DECODER": "openjpeg"}, None),
    "spike": ((4, 32, 32), ["-D", "2"], {}, None, {}, _spike),
}


class Case:
    pass


_BUILT = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("window")


def case(name, workdir):
    """Encode + whole decode of one case, once per module."""
    if name in _BUILT:
        return _BUILT[name]
    import decode
    import encode
    from lbdrn_hip import container, raster_io
    from lbdrn_hip.features import FeatCfg
    from lbdrn_hip.synth import synthetic_tile
    shape, flags, consts, base_codec, env, hook = CASES[name]
    c = Case()
    c.name, c.consts, c.env = name, consts, env
    c.img = synthetic_tile(3 + list(CASES).index(name), *shape)
    if hook is not None:
        c.img = hook(c.img)
    c.src = str(workdir / f"{name}.npy")
    np.save(c.src, c.img)
    out = workdir / name
    with _settings(consts, base_codec, env):
        assert encode.main(["-i", c.src, "-o", str(out), "-e", "1", "-bs", "512"] + flags) == 0
        (sub,) = [d for d in out.iterdir() if d.is_dir()]
        c.dir, c.bin = sub, str(sub / f"{name}.bin")
        assert decode.main(["-i", c.bin]) == 0
    c.raw = open(c.bin, "rb").read()
    c.full = raster_io.read_raster(str(sub / f"{name}_recon.tif")).reshape(shape)
    c.full_bytes = open(str(sub / f"{name}_recon.tif"), "rb").read()
    c.log = _records(sub / "decode.txt")
    c.n_hdr, c.sr, c.width, c.height, c.K, c.bc, c.nl, c.D, c.nn, c.base = container.unpack_header(c.raw)
    assert (c.width, c.height) == (shape[2], shape[1]) and np.array_equal(c.full >> c.K, c.img >> c.K)
    # what decode.py's FeatCfg.from_constants() gave while the switches were set; the activation comes from the header
    c.cfg = FeatCfg(use_coordinates=consts.get("USE_COORDINATES", False), embedding=consts.get("EMBEDDING", False))
    _BUILT[name] = c
    return c


def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f]


def windows(c):
    """The windows of one case (x0, y0, w, h): whole scene, corners, interior pixel, flush with each edge, D-1 / D / D+1
    from a tile edge on either side of it, across tile boundaries, ten random ones."""
    from LBDRNdataset import tile_windows
    W, H, D = c.width, c.height, c.D
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (W // 2 + 1, H // 2 - 1, 1, 1),
           (0, 3, 5, 4), (W - 5, 3, 5, 4), (3, 0, 4, 5), (3, H - 5, 4, 5)]
    tiles = list(tile_windows(W, H, c.sr))
    _, _, tx, ty, tw, th = tiles[-1] if c.sr == 1 else tiles[c.sr + 1]       # (with tiles: one with neighbours up and left)
    for d in sorted({max(D - 1, 0), D, D + 1}):
        out.append((tx + d, ty + d, 3, 2))                                    # d inside the tile's left / top edge
        out.append((tx + tw - d - 3, ty + th - d - 2, 3, 2))                  # d inside its right / bottom edge
        if c.sr > 1:
            out.append((tx - d - 2, ty - d - 2, 2, 2))                        # d outside: in the neighbours
            out.append((tx - d - 1, ty + 1, d + 3, 2))                        # from d + 1 outside to 2 inside
    if c.sr > 1:
        out += [(tx - 3, ty + 2, 7, 2), (tx + 2, ty - 3, 2, 7), (tx - 1, ty - 1, 2, 2), (1, 1, W - 2, H - 2)]
    rng = np.random.default_rng(len(c.name) * 1000 + W)
    for _ in range(10):
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x0, y0, int(rng.integers(1, W - x0 + 1)), int(rng.integers(1, H - y0 + 1))))
    return out


def _paths():
    from lbdrn_hip import ops
    return (("generic", ops._lib.PATH_GENERIC), ("mfma", ops._lib.PATH_MFMA), ("auto", ops.PATH_AUTO))


def has_mfma_kernel(c, dev):
    """Whether the whole-tile apply of this file runs under PATH_MFMA (codec.apply_image on tile 0's payloads)."""
    from lbdrn_hip import codec, container, ops
    from lbdrn_hip.features import FeatCfg
    cfg = FeatCfg(c.cfg.use_coordinates, c.cfg.embedding, activation=container.header_activation(c.raw) or "sine")
    params = container.decode_weights(c.raw[c.n_hdr:c.n_hdr + c.nn[0]])
    msb = container.decode_base(c.raw[c.n_hdr + c.nn[0]:c.n_hdr + c.nn[0] + c.base[0]], device=str(dev))
    try:
        codec.apply_image(msb, params, c.K, c.D, c.bc, c.nl, cfg=cfg, device=str(dev), path=ops._lib.PATH_MFMA)
    except ops._lib.LbdrnError:
        return False
    return True


def check_windows(c, dev, paths=None):
    from lbdrn_hip import codec, ops
    wins = windows(c)
    with _settings(c.consts, None, c.env):
        for pname, path in paths or _paths():
            if pname == "mfma" and not has_mfma_kernel(c, dev):     # no quiet fall-back on a crop either
                with pytest.raises(ops._lib.LbdrnError):
                    codec.decode_window(c.raw, wins[0], device=str(dev), path=path, cfg=c.cfg)
                continue
            for win in wins:
                x0, y0, w, h = win
                got = codec.decode_window(c.raw, win, device=str(dev), path=path, cfg=c.cfg, keep_on_device=False)
                assert got.dtype == np.uint16 and got.shape == (c.full.shape[0], h, w), (c.name, pname, win)
                assert np.array_equal(got, c.full[:, y0:y0 + h, x0:x0 + w]), (c.name, pname, win)
    return len(wins)


@pytest.mark.parametrize("name", ("headline", "ragged", "nine", "generic", "embed", "coords", "relu", "wide"))
def test_windows_equal_the_crop_of_the_whole_decode(name, dev, workdir):
    c = case(name, workdir)
    assert check_windows(c, dev) >= 24
    if name == "relu":
        from lbdrn_hip import container
        assert container.header_activation(c.raw) == "relu"       # (c.cfg says sine: the header wins, as in decode.py)
    if name in ("headline", "wide"):
        assert c.bc == (256 if name == "wide" else 64) and has_mfma_kernel(c, dev)      # k_apply_mfma / k_apply_wide ran
    if name == "nine":
        assert c.sr == 3 and len(c.nn) == 9


def test_windows_of_a_gpu_coded_jpeg2000_payload(dev, workdir):
    from lbdrn_hip import jp2
    c = case("jp2gpu", workdir)
    assert jp2.is_jp2(c.raw[c.n_hdr + c.nn[0]:c.n_hdr + c.nn[0] + c.base[0]])
    check_windows(c, dev)


def test_windows_of_an_openjpeg_payload(dev, workdir):
    from lbdrn_hip import jp2
    if not jp2.available():
        pytest.skip("liblbdrn_jp2.so is not built here (no OpenJPEG)")
    c = case("jp2", workdir)
    assert jp2.is_jp2(c.raw[c.n_hdr + c.nn[0]:c.n_hdr + c.nn[0] + c.base[0]])
    check_windows(c, dev)


def test_device_tensor_is_the_default_result(dev, workdir):
    import torch
    from lbdrn_hip import codec, ops
    c = case("headline", workdir)
    t = codec.decode_window(c.raw, (7, 9, 20, 11), device=str(dev))
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (8, 11, 20)
    assert np.array_equal(ops.from_device_u16(t), c.full[:, 9:20, 7:27])
    with pytest.raises(ValueError, match="52 x 40"):
        codec.decode_window(c.raw, (50, 0, 3, 1), device=str(dev))


def test_untouched_tiles_are_not_read(dev, workdir):
    """-sr 3: with the payload bytes of every tile the window does not touch overwritten, the window decodes to the same
    bits; with a touched tile's overwritten instead, the decode raises."""
    from lbdrn_hip import codec
    c = case("nine", workdir)
    offsets = [c.n_hdr]
    for t in range(9):
        offsets.append(offsets[-1] + c.nn[t] + c.base[t])
    assert offsets[-1] == len(c.raw)
    for win in ((18, 20, 9, 8), (2, 3, 5, 6), (30, 10, 10, 25), (14, 14, 20, 20)):
        x0, y0, w, h = win
        touched = [p.tile for p in codec.window_pieces(c.width, c.height, 3, win, c.D)]
        assert 0 < len(touched) and (len(touched) < 9 or win == (14, 14, 20, 20))
        dirty = bytearray(c.raw)
        for t in range(9):
            if t not in touched:
                dirty[offsets[t]:offsets[t + 1]] = b"\xA5" * (offsets[t + 1] - offsets[t])
        assert len(touched) == 9 or bytes(dirty) != c.raw
        got = codec.decode_window(bytes(dirty), win, device=str(dev), cfg=c.cfg, keep_on_device=False)
        assert np.array_equal(got, c.full[:, y0:y0 + h, x0:x0 + w]), win
        dirty = bytearray(c.raw)
        t = touched[-1]
        dirty[offsets[t]:offsets[t + 1]] = b"\xA5" * (offsets[t + 1] - offsets[t])
        with pytest.raises(Exception):
            codec.decode_window(bytes(dirty), win, device=str(dev), cfg=c.cfg, keep_on_device=False)


def test_the_normaliser_is_the_whole_tiles_maximum(dev, workdir):
    """The tile's largest MSB value lies outside the window: a crop-derived MSB.max() gives other bits."""
    from lbdrn_hip import codec, container
    c = case("spike", workdir)
    msb = container.decode_base(c.raw[c.n_hdr + c.nn[0]:])
    win = (3, 4, 17, 13)
    x0, y0, w, h = win
    m = c.D
    assert int(msb[:, y0 - m:y0 + h + m, x0 - m:x0 + w + m].max()) < int(msb.max()) == 60000 >> c.K
    for pname, path in _paths():
        got = codec.decode_window(c.raw, win, device=str(dev), path=path, keep_on_device=False)
        assert np.array_equal(got, c.full[:, y0:y0 + h, x0:x0 + w]), pname
    # the trap is real for this image: the same crop under its own maximum decodes to other low bits
    params = container.decode_weights(c.raw[c.n_hdr:c.n_hdr + c.nn[0]])
    crop = np.ascontiguousarray(msb[:, y0 - m:y0 + h + m, x0 - m:x0 + w + m])
    wrong = codec.apply_image(crop, params, c.K, c.D, c.bc, c.nl, device=str(dev))[:, m:m + h, m:m + w]
    assert not np.array_equal(wrong, c.full[:, y0:y0 + h, x0:x0 + w])
    check_windows(c, dev, paths=_paths()[2:])


def test_the_command_line(dev, workdir, capsys):
    """--window writes the crop of the whole _recon.tif; -org logs the window's MSE; a run without --window gives the bytes
    and the records of the whole decode made for the module."""
    import decode
    from lbdrn_hip import raster_io
    c = case("ragged", workdir)
    marker = (c.dir / "decode.txt").read_text()
    with _settings(c.consts, None, c.env):
        for win in ((20, 11, 10, 30), (0, 0, 37, 50), (36, 49, 1, 1)):
            x0, y0, w, h = win
            assert decode.main(["-i", c.bin, "--window"] + [str(v) for v in win] + ["-org", c.src]) == 0
            path = c.dir / f"ragged_recon_x{x0}_y{y0}_w{w}_h{h}.tif"
            rec = raster_io.read_raster(str(path)).reshape(4, h, w)
            assert np.array_equal(rec, c.full[:, y0:y0 + h, x0:x0 + w])
            recs = _records(c.dir / "decode_window.txt")
            assert [r.split(":")[0] for r in recs] == ["Binstream", "Window", "Recon", "Time elapsed", "MSE", "PSNR"]
            assert recs[1] == f"Window: x0={x0} y0={y0} w={w} h={h} of 37 x 50"
            a, b = c.img[:, y0:y0 + h, x0:x0 + w], c.full[:, y0:y0 + h, x0:x0 + w]
            mse = np.mean((a.astype(np.float32) - b.astype(np.float32)) ** 2)
            assert recs[4] == f"MSE: {mse}" and recs[5] == f"PSNR: {10 * np.log10(10000 ** 2 / mse)}"
            assert (c.dir / "decode.txt").read_text() == marker
        other = str(workdir / "elsewhere.tif")
        assert decode.main(["-i", c.bin, "--window", "5", "6", "7", "8", "-o", other]) == 0
        assert np.array_equal(raster_io.read_raster(other), c.full[:, 6:14, 5:12])
        # without the flag: today's decode
        os.remove(str(c.dir / "ragged_recon.tif"))
        assert decode.main(["-i", c.bin]) == 0
        assert open(str(c.dir / "ragged_recon.tif"), "rb").read() == c.full_bytes
        strip = lambda recs: [r for r in recs if not r.startswith("Time elapsed")]
        assert strip(_records(c.dir / "decode.txt")) == strip(c.log) and len(c.log) == 2
