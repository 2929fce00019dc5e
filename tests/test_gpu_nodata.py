"""encode.py --nodata / decode.py on the GPU: lbdrn_hip.nodata.tile_mask and apply against tests/nodata_reference.py on the
shapes at which the plane coder under them changes path, and the command lines end to end on the reference-made learnable
4 x 256 x 256 raster and on a 70 x 131 crop of it at -sr 2: decoded == V exactly where original == V, whatever K, T, the MSB
codec and the activation are, for a whole decode and for a window.  Every comparison is exact.

The prepared raster (prepare): every valid sample that equals V is moved off it, a diagonal collar is set to V in all bands
(one sample more in one band: that tile's masks differ between bands), and a few VALID samples of V +- 1 and V +- 2 are planted
deep inside the collar.  A planted value that has V's high bits leaves the MSB planes flat around it, and with relative colours
a flat neighbourhood is the all-zero feature vector: the base decode of such a sample is exactly what it is for the collar's
own samples of that band.  So wherever the fit reproduces the collar in a band -- which is what it is trained to do on
thousands of identical rows -- every planted sample of that band decodes to V and has to be bumped.  The K = 1 case leaves
the network one bit to predict there.  test_some_case_bumps_a_planted_sample asserts that this happened."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nodata_reference as N  # noqa: E402
import pyramid_reference as PR  # noqa: E402
import tiff_reference as TR  # noqa: E402
from pyramid_helpers import GEO, with_tags  # noqa: E402
from test_gpu_window_decode import _records, _settings  # noqa: E402

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- tile_mask / apply

SHAPES = ((1, 1, 1), (3, 65, 130), (8, 70, 257))      # one sample; a strip edge at 64 columns, a pass edge at 64 rows; a ragged last strip
KINDS = (0, 1, 2, 3)
RECTS = ((0, 0, 1, 1), (-1, 0, 1, 1), (0, -1, 1, 1), (-1, -1, 1, 1), (60, 60, 9, 9), (63, 0, 2, 65), (0, 63, 66, 2), (64, 64, 1, 1),
         (1, 2, 127, 62), (128, 0, 2, 3))      # negative: counted from the far edge; clipped to the shape


def _original(shape, kind, V, seed):
    """planes whose mask against V is of `kind`; valid samples lie within 3 of V"""
    rng = np.random.default_rng(seed)
    C, H, W = shape
    a = (V + rng.integers(1, 4, shape) * (1 if V < 60000 else -1)).astype(np.uint16)
    if kind == 1:
        a[:] = V
    elif kind >= 2:
        yy, xx = np.mgrid[0:H, 0:W]
        a[:, (yy * 3 + xx * 2) % 7 < 3] = V
        a[:, : H // 2, : W // 3] = V
        if kind == 3:
            a[C - 1, H - 1, W - 1] = V if a[C - 1, H - 1, W - 1] != V else N.bump_value(V)      # one band's mask differs in one sample
    return a


def _possible(shape, kind):
    return kind < 2 or (shape != (1, 1, 1) and (kind == 2 or shape[0] > 1))


@pytest.mark.parametrize("V", (0, 1000, 65535))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tile_mask_and_apply_equal_the_reference(dev, shape, kind, V):
    from lbdrn_hip import container, nodata, ops
    if not _possible(shape, kind):
        return      # (one sample is nodata or is not: there are no kinds 2 and 3 of it)
    C, H, W = shape
    orig = _original(shape, kind, V, 7 * kind + sum(shape))
    want_kind, planes = N.tile_kind(orig, V)
    assert want_kind == kind
    got_kind, body, count = nodata.tile_mask(ops.to_device_u16(orig, dev), V)
    assert (got_kind, count) == (kind, int((orig == V).sum()))
    if kind < 2:
        assert body == b""
    else:
        assert planes.shape == ((1 if kind == 2 else C), H, W)
        assert body == container.encode_base(planes, codec="LBB2", device=dev) and body[:4] == b"LBB2"
        assert np.array_equal(container.decode_base(body, device=dev), planes)
    # the mask step on a reconstruction that holds V, its neighbours and the bump's target among valid and nodata samples alike
    rng = np.random.default_rng(11 + sum(shape))
    lo = max(0, V - 2)
    r1 = rng.integers(lo, min(65535, V + 2) + 1, shape).astype(np.uint16)
    want = N.mask_step(r1, orig == V, V).astype(np.uint16)
    got = ops.from_device_u16(nodata.apply(ops.to_device_u16(r1, dev), kind, body, V))
    assert np.array_equal(got, want)
    assert np.array_equal(got == V, orig == V)
    if kind != 1 and orig.size > 1:
        assert ((orig != V) & (r1 == V)).any() and (got[(orig != V) & (r1 == V)] == N.bump_value(V)).all()
    # rectangles: the same result as the crop of the whole
    for x0, y0, w, h in RECTS:
        x0, y0 = (x0 if x0 >= 0 else W + x0), (y0 if y0 >= 0 else H + y0)
        if x0 >= W or y0 >= H:
            continue
        w, h = min(w, W - x0), min(h, H - y0)
        crop = np.ascontiguousarray(r1[:, y0:y0 + h, x0:x0 + w])
        part = ops.from_device_u16(nodata.apply(ops.to_device_u16(crop, dev), kind, body, V, (x0, y0, w, h)))
        assert np.array_equal(part, want[:, y0:y0 + h, x0:x0 + w]), (x0, y0, w, h)


def test_apply_refuses_planes_and_rectangles_that_do_not_fit_the_mask(dev):
    from lbdrn_hip import nodata, ops
    orig = _original((3, 65, 130), 3, 0, 1)
    kind, body, _ = nodata.tile_mask(ops.to_device_u16(orig, dev), 0)
    for planes, rect in ((orig[:, :64], None), (orig[:2], None), (orig[:, :4, :4], (0, 0, 5, 4)), (orig[:, :4, :4], (127, 0, 4, 4)),
                         (orig[:, :4, :4], (0, 62, 4, 4))):
        with pytest.raises(ValueError):
            nodata.apply(ops.to_device_u16(np.ascontiguousarray(planes), dev), kind, body, 0, rect)
    with pytest.raises(ValueError):
        nodata.apply(ops.to_device_u16(orig, dev), 2, body, 0)      # three planes where the kind says one
    with pytest.raises(ValueError):
        nodata.tile_mask(ops.to_device_u16(orig, dev), 65536)


# ---------------------------------------------------------------- the command lines

def prepare(img, V, K, extra=True):
    """-> (the raster, [(band, y, x)] of the planted valid samples whose MSB is V's)"""
    a = img.astype(np.uint16).copy()
    a[a == V] = N.bump_value(V)                       # 1. no valid sample equals V
    C, H, W = a.shape
    yy, xx = np.mgrid[0:H, 0:W]
    a[:, yy + xx < (H + W) * 3 // 10] = V             # 2. the collar
    if extra:
        a[1, H - 1, W - 1] = V
    planted = []
    values = [V + 1, V + 2] + ([V - 1, V - 2] if V >= 2 else [])
    for c in range(C):                                # 3. valid samples next to V, deep inside the collar, 6 apart
        for j, v in enumerate(values):
            y, x = 3 + 6 * j, 3 + 6 * c
            assert y + x + 2 * 2 < (H + W) * 3 // 10
            a[c, y, x] = v
            if v >> K == V >> K:
                planted.append((c, y, x))
    return a, planted


CASES = {      # V, T, K, crop (else the whole raster), -sr, MSB codec, constants, environment
    "v0": (0, None, 5, False, 1, "LBB2", {}, {}),
    "v0-t0": (0, 0, 5, False, 1, "LBB2", {}, {}),
    "v0-t2": (0, 2, 5, False, 1, "LBB2", {}, {}),
    "v1000": (1000, None, 5, False, 1, "LBB2", {}, {}),
    "v1000-t0": (1000, 0, 5, False, 1, "LBB2", {}, {}),
    "v1000-t2": (1000, 2, 5, False, 1, "LBB2", {}, {}),
    "crop-sr2-lbb3": (0, 2, 5, True, 2, "LBB3", {}, {}),
    "crop-sr2-relu": (1000, None, 5, True, 2, "LBB2", {"HIDDEN_ACTIVATION": "relu"}, {}),
    "crop-sr2-k1": (1000, None, 1, True, 2, "LBB2", {}, {}),
    "crop-sr2-k1-t2": (0, 2, 1, True, 2, "LBB2", {}, {}),
}
_DONE = {}


class Result:
    pass


def _decode(binp, flags, shape, out=None):
    import decode
    from lbdrn_hip import raster_io
    d = os.path.dirname(binp)
    for log in ("decode.txt", "decode_window.txt"):
        if os.path.exists(os.path.join(d, log)):
            os.remove(os.path.join(d, log))
    assert decode.main(["-i", binp] + flags + (["-o", out] if out else [])) == 0
    path = out or binp[:-4] + "_recon.tif"
    return raster_io.read_raster(path).reshape(shape), path


def run_case(name, golden, work):
    """the case's encode (with the flag, and without it where there is no layer) and its decodes; once per module"""
    if name in _DONE:
        return _DONE[name]
    import encode
    from lbdrn_hip import container
    V, T, K, crop, sr, codec, consts, env = CASES[name]
    img = golden["rasters_learn_bands4"]["img"]
    assert img.shape == (4, 256, 256)
    if crop:
        img = np.ascontiguousarray(img[:, 100:170, 60:191])
        assert img.shape == (4, 70, 131)
    r = Result()
    r.V, r.T, r.K = V, T, K
    r.img, r.planted = prepare(img, V, K)
    src = str(work / f"{name}.npy")
    np.save(src, r.img)
    common = ["-i", src, "-e", "2", "-bs", "8192" if not crop else "512", "-K", str(K), "-sr", str(sr)]
    layer = ["--max-error", str(T)] if T is not None else []
    r.window = (2, 1, 120, 100) if not crop else (2, 1, 100, 50)
    x0, y0, w, h = r.window
    with _settings(consts, codec, env):
        assert encode.main(common + ["-o", str(work / name), "--nodata", str(V)] + layer) == 0
        (sub,) = [d for d in (work / name).iterdir() if d.is_dir()]
        r.bin, r.log = str(sub / f"{name}.bin"), str(sub / "encode.txt")
        r.raw = open(r.bin, "rb").read()
        r.old = None
        if T is None:
            assert encode.main(common + ["-o", str(work / (name + "-old"))]) == 0
            (old,) = [d for d in (work / (name + "-old")).iterdir() if d.is_dir()]
            r.old = open(str(old / f"{name}.bin"), "rb").read()
        r.full, r.full_path = _decode(r.bin, [], r.img.shape)
        r.decode_records = _records(os.path.join(os.path.dirname(r.bin), "decode.txt"))
        r.nomask, _ = _decode(r.bin, ["--no-mask"], r.img.shape)
        r.base, _ = _decode(r.bin, ["--no-mask", "--no-enhancement"], r.img.shape)
        win = ["--window"] + [str(v) for v in r.window]
        r.win, _ = _decode(r.bin, win, (4, h, w), str(work / f"{name}-window.tif"))
        r.win_nomask, _ = _decode(r.bin, win + ["--no-mask"], (4, h, w), str(work / f"{name}-window-nomask.tif"))
    r.chunk, r.layer = container.unpack_nodata_trailer(r.raw), container.unpack_residual_trailer(r.raw)
    _DONE[name] = r
    return r


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("nodata")


@pytest.mark.parametrize("name", list(CASES))
def test_encode_decode_end_to_end(golden, dev, work, name):
    from lbdrn_hip import container
    r = run_case(name, golden, work)
    V, T, img = r.V, r.T, r.img.astype(np.int64)
    nod = img == V
    assert nod.any() and not nod.all()
    # decoded == V exactly when original == V: the whole decode and the window
    assert np.array_equal(r.full == V, nod)
    x0, y0, w, h = r.window
    assert np.array_equal(r.win, r.full[:, y0:y0 + h, x0:x0 + w])
    assert np.array_equal(r.win_nomask, r.nomask[:, y0:y0 + h, x0:x0 + w])
    # the --no-mask decode everywhere else, except the bumped samples, which go one count off V
    bumped = ~nod & (r.nomask == V)
    assert np.array_equal(r.full[~nod & ~bumped], r.nomask[~nod & ~bumped])
    assert (r.full[bumped] == N.bump_value(V)).all()
    r.bumped = int(bumped.sum())
    r.bumped_planted = sum(bool(bumped[p]) for p in r.planted)
    # the planted samples that share V's high bits decode, at the base, to what the collar decodes to in their band
    assert r.planted
    for c, y, x in r.planted:
        assert r.base[c, y, x] == r.base[c, 1, 1], (c, y, x)
    # the layer: the stored tau is the rule's, the bound holds on every sample, T = 0 is lossless, nodata samples cost nothing
    if T is None:
        assert r.layer is None and np.array_equal(r.nomask, r.base)
        assert r.raw[:len(r.old)] == r.old and r.raw[len(r.old):] == container.pack_nodata_trailer(*r.chunk)      # today's file + one chunk
    else:
        assert r.layer[0] == N.tau_for(T, V)
        assert int(np.abs(img - r.full).max()) <= T
        assert T or np.array_equal(r.full, r.img)
        assert np.array_equal(r.nomask[nod], r.base[nod])
        want, _, _ = N.chain(img, r.base, V, T)
        assert np.array_equal(r.full, want)
    want, _, _ = N.chain(img, r.nomask, V, None)
    assert np.array_equal(r.full, want)
    # the chunk and the records
    assert r.chunk[0] == V and len(r.chunk[1]) == CASES[name][4] ** 2
    kinds = [k for k, _ in r.chunk[1]]
    assert 3 in kinds and (CASES[name][4] == 1 or len(set(kinds)) > 1)
    recs = [x for x in _records(r.log) if x.startswith("Nodata: ")]
    assert len(recs) == len(kinds) + 1 and recs[-1].startswith(f"Nodata: V={V}, {int(nod.sum())} samples, mask ")
    assert f"Nodata: V={V}" in r.decode_records
    assert container.header_activation(r.raw) == ("relu" if "relu" in name else None)


def test_some_case_bumps_a_planted_sample(golden, dev, work):
    """the coverage condition: the bump is taken, and by a planted sample, in at least one case"""
    got = {}
    for name in CASES:
        r = run_case(name, golden, work)
        nod = r.img == r.V
        bumped = ~nod & (r.nomask == r.V)
        got[name] = (int(bumped.sum()), sum(bool(bumped[p]) for p in r.planted))
    print("bumped samples (all, planted) per case:", got)
    assert any(n for n, _ in got.values()), got
    assert any(p for _, p in got.values()), got


def test_k_in_flight_files_equal_the_point_after_point_ones(golden, dev, work, monkeypatch):
    import encode
    img, _ = prepare(np.ascontiguousarray(golden["rasters_learn_bands4"]["img"][:, 100:170, 60:191]), 0, 5)
    src = str(work / "sweep.npy")
    np.save(src, img)
    monkeypatch.setattr(encode, "BASE_CODEC", "LBB2")
    monkeypatch.setattr(encode, "DEVICE", "cuda:0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    Ks = (4, 5)
    for tag, extra in (("plain", []), ("layer", ["--max-error", "2"])):
        flags = ["-i", src, "-e", "2", "-bs", "512", "-sr", "2", "--nodata", "0"] + extra
        for K in Ks:
            assert encode.main(flags + ["-o", str(work / f"one-{tag}"), "-K", str(K)], shard_tiles=False) == 0
        assert encode.main_k_points(flags + ["-o", str(work / f"many-{tag}")], Ks) == {K: None for K in Ks}
        chunks = set()
        for K in Ks:
            sub = f"sweep_r2_K{K}_bc64_nl2_D2_prec16_lr0.001_bs512_e2"
            a, b = ((work / f"{d}-{tag}" / sub / "sweep.bin").read_bytes() for d in ("one", "many"))
            assert a == b
            from lbdrn_hip import container
            chunks.add(container.pack_nodata_trailer(*container.unpack_nodata_trailer(a)))
        assert len(chunks) == 1      # the mask does not depend on K


def _tiff(path, img, tags):
    data = TR.write_tiff(img, rows_per_strip=8)[0]
    with open(path, "wb") as f:
        f.write(with_tags(data, tags) if tags else data)
    return str(path)


def test_overviews_take_the_chunk_s_value_and_the_output_names_it(golden, dev, work):
    """--out-overviews: --out-nodata, then the chunk's V, then a stored GDAL_NODATA; a TIFF output without a GDAL_NODATA from
    stored or copied tags gets one that names V"""
    import encode
    from lbdrn_hip import geotags, raster_io
    r = run_case("v1000-t0", golden, work)
    _, path = _decode(r.bin, [], r.img.shape)
    assert raster_io.read_geo_tags(path) == [(42113, 2, 5, b"1000\0")]
    _, path = _decode(r.bin, ["--no-mask"], r.img.shape)
    assert raster_io.read_geo_tags(path) == []
    flags = ["--out-compress", "deflate", "--out-tile", "64", "--out-overviews", "2"]
    _, path = _decode(r.bin, flags, r.img.shape)
    assert geotags.stored_nodata(raster_io.read_geo_tags(path), 16) == 1000
    implied = [raster_io.read_raster(path, overview=k) for k in (0, 1, 2)]
    assert np.array_equal(implied[0], r.img)
    for k, level in enumerate(PR.pyramid(r.img, 2, "average", 1000), 1):      # samples of 1000 do not enter an average
        assert np.array_equal(implied[k], level)
    _, path = _decode(r.bin, flags + ["--out-nodata", "1000"], r.img.shape)
    for k in (1, 2):
        assert np.array_equal(raster_io.read_raster(path, overview=k), implied[k])
    _, path = _decode(r.bin, flags + ["--out-nodata", "7"], r.img.shape)                      # --out-nodata wins
    assert not np.array_equal(raster_io.read_raster(path, overview=1), implied[1])
    assert geotags.stored_nodata(raster_io.read_geo_tags(path), 16) == 1000
    # a scene whose tag names another value than the flag: the chunk's V is the overviews' nodata, the stored tag stays on the output
    tags = [GEO[0], GEO[1], (42113, 2, 4, b"255\0")]
    img = r.img[:, :70, :131]
    src = _tiff(work / "tagged.tif", img, tags)
    with _settings(None, "LBB2", None):
        assert encode.main(["-i", src, "-o", str(work / "tagged"), "-e", "1", "-bs", "512", "--nodata", "1000", "--max-error", "0", "--keep-tags"]) == 0
        (sub,) = [d for d in (work / "tagged").iterdir() if d.is_dir()]
        binp = str(sub / "tagged.bin")
        flags = ["--out-compress", "deflate", "--out-tile", "16", "--out-overviews", "1"]
        _, path = _decode(binp, flags, img.shape)
        assert raster_io.read_geo_tags(path) == tags
        by_chunk = raster_io.read_raster(path, overview=1)
        _, path = _decode(binp, flags + ["--out-nodata", "1000"], img.shape)
        assert np.array_equal(raster_io.read_raster(path, overview=1), by_chunk)
        _, path = _decode(binp, flags + ["--no-mask"], img.shape)                             # without the chunk: the stored 255
        assert not np.array_equal(raster_io.read_raster(path, overview=1), by_chunk)
        # --nodata tag takes the scene's 255
        assert encode.main(["-i", src, "-o", str(work / "by-tag"), "-e", "1", "-bs", "512", "--nodata", "tag"]) == 0
        (sub,) = [d for d in (work / "by-tag").iterdir() if d.is_dir()]
        from lbdrn_hip import container
        assert container.unpack_nodata_trailer(open(str(sub / "tagged.bin"), "rb").read())[0] == 255
