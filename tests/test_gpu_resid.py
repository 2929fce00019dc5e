"""liblbdrn_resid.so on the GPU (include/lbdrn_resid.h): body bytes and decoded rasters against tests/resid_reference.py for
every geometry class, the extremes, rectangles that must skip the blocks they do not touch, refusals and damaged bodies
behind guard bands (tests/guarded.py), and encode.py --max-error / decode.py end to end on the reference-made learnable
4 x 256 x 256 raster.  Every comparison is exact; damaged inputs are only ever supplied, never a fault provoked."""
import contextlib
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import resid_reference as R  # noqa: E402
from guarded import Arena  # noqa: E402
from test_resid_host import GEOMETRIES, random_planes  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG, E_WORKSPACE = -1, -4
_cache = {}


def _lib():
    from lbdrn_hip import resid
    return resid.lib()


def _stream(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def reference(key, make):
    """(orig, recon, {tau: (body, recon')}): computed once per key, shared and never changed"""
    if key not in _cache:
        orig, recon = make()
        _cache[key] = (orig, recon, {})
    return _cache[key]


def ref_body(key, make, tau):
    orig, recon, bodies = reference(key, make)
    if tau not in bodies:
        bodies[tau] = R.encode_body(orig, recon, tau)
    return orig, recon, bodies[tau][0], bodies[tau][1]


def gpu_encode(dev, orig, recon, tau, fill):
    """lbdrn_resid_encode into guarded buffers -> body bytes"""
    import torch
    L = _lib()
    C, H, W = orig.shape
    A = Arena(dev)
    o, r = A.const(orig, "orig"), A.const(recon, "recon")
    cap, nws = L.lbdrn_resid_bound(C, H, W), L.lbdrn_resid_workspace(C, H, W)
    body, nb, ws = A.buf(cap, fill, name="body"), A.buf(8, fill, name="body_bytes"), A.buf(nws, fill, name="workspace")
    rc = L.lbdrn_resid_encode(o.ptr, r.ptr, C, H, W, tau, body.ptr, cap, nb.ptr, ws.ptr, nws, _stream(dev))
    assert rc == 0, L.lbdrn_resid_last_error()
    torch.cuda.synchronize()
    A.check()
    n = int(nb.numpy(np.int64)[0])
    assert 0 < n <= cap
    return body.numpy(np.uint8, n).tobytes()


def gpu_decode(dev, body, C, H, W, recon_rect, rect, fill):
    """lbdrn_resid_decode on guarded buffers -> (host return code, status, planes of the rectangle)"""
    import torch
    L = _lib()
    x0, y0, w, h = rect
    A = Arena(dev)
    b = A.const(np.frombuffer(body, np.uint8), "body")
    rec = A.buf(recon_rect.nbytes, fill, name="recon").write(recon_rect)
    nws = L.lbdrn_resid_decode_workspace(C, H, W)
    st, ws = A.buf(4, fill, name="status"), A.buf(nws, fill, name="workspace")
    rc = L.lbdrn_resid_decode(b.ptr, len(body), C, H, W, x0, y0, w, h, rec.ptr, st.ptr, ws.ptr, nws, _stream(dev))
    torch.cuda.synchronize()
    A.check()
    return rc, (int(st.numpy(np.int32)[0]) if rc == 0 else None), rec.numpy(np.uint16).reshape(C, h, w)


def first_difference(got, want, C, H, W):
    """names the first differing block (and row, where the row tables differ) of two bodies"""
    try:
        _, _, _, _, eg = R.parse_tables(got)
        _, _, _, _, ew = R.parse_tables(want)
    except R.Damaged as e:
        return f"the product's body does not parse: {e}"
    for k, ((c, y0, x0, rows, cols), (og, ng), (ow, nw)) in enumerate(zip(R.blocks_of(C, H, W), eg, ew)):
        bg, bw = got[og:og + ng], want[ow:ow + nw]
        if bg != bw:
            lg, lw = struct.unpack(f"<{rows}H", bg[:2 * rows]), struct.unpack(f"<{rows}H", bw[:2 * rows])
            row = next((r for r in range(rows) if lg[r] != lw[r]), None)
            if row is None:
                ug, uw = R.decode_block(bg, rows, cols), R.decode_block(bw, rows, cols)
                row = int(np.flatnonzero((ug != uw).any(axis=1))[0])
            return f"block {k} (plane {c}, y0 {y0}, x0 {x0}), row {row}"
    return "header or block table"


# ---------------------------------------------------------------- geometries

@pytest.mark.parametrize("tau", [0, 1, 3])
@pytest.mark.parametrize("shape", GEOMETRIES, ids=lambda s: "x".join(map(str, s)))
def test_body_and_decode_equal_the_reference(dev, shape, tau):
    C, H, W = shape
    orig, recon, want_body, want = ref_body(shape, lambda: random_planes(np.random.default_rng(sum(shape)), C, H, W), tau)
    for fill in (0xA5, 0x00):
        body = gpu_encode(dev, orig, recon, tau, fill)
        assert body == want_body, f"{shape} tau {tau}: first difference in {first_difference(body, want_body, C, H, W)}"
        rc, status, rec = gpu_decode(dev, body, C, H, W, recon, (0, 0, W, H), fill)
        assert rc == 0 and status == 0
        assert np.array_equal(rec, want)
    assert int(np.abs(want.astype(np.int64) - orig).max()) <= tau


# ---------------------------------------------------------------- extremes

def _extremes():
    C, H, W = 1, 70, 300
    z, m = np.zeros((C, H, W), np.uint16), np.full((C, H, W), 65535, np.uint16)
    alt = z.copy()
    alt[:, :, 1::2] = 65535
    rng = np.random.default_rng(9)
    mixed = rng.integers(0, 3, (C, H, W)).astype(np.uint16)
    mixed[:, :, ::7] = 65535            # rows of small values with extremes among them: the escape is taken
    return {"up": (m, z, 0), "down": (z, m, 0), "equal": (alt, alt.copy(), 0), "all-in-tau": (m, z, 65535),
            "columns": (alt, 65535 - alt, 0), "columns tau 2": (alt, 65535 - alt, 2), "escapes": (mixed, z, 0)}


@pytest.mark.parametrize("name", list(_extremes()))
def test_extremes(dev, name):
    orig, recon, tau = _extremes()[name]
    C, H, W = orig.shape
    want_body, want = R.encode_body(orig, recon, tau)
    body = gpu_encode(dev, orig, recon, tau, 0xA5)
    assert body == want_body, first_difference(body, want_body, C, H, W)
    rc, status, rec = gpu_decode(dev, body, C, H, W, recon, (0, 0, W, H), 0xA5)
    assert rc == 0 and status == 0 and np.array_equal(rec, want)
    assert int(np.abs(rec.astype(np.int64) - orig).max()) <= tau
    nblocks = C * 2 * 2
    if name in ("equal", "all-in-tau"):       # every row empty: the header, the table and the row lengths
        assert len(body) == 20 + 4 * nblocks + 2 * 2 * C * H
    if name == "escapes":
        k = int(R.encode_row(R.fold(R.quantise(orig[0, 0, :256], recon[0, 0, :256], 0)))[:4], 2)
        assert (65535 * 2) >> k >= 24


# ---------------------------------------------------------------- rectangles

RECTS = {"one sample": (300, 70, 1, 1), "block corner": (250, 60, 20, 8), "one full block": (256, 64, 256, 64),
         "last partial column": (512, 0, 3, 130), "whole tile": (0, 0, 515, 130)}


@pytest.mark.parametrize("name", list(RECTS))
def test_rectangles_decode_only_their_blocks(dev, name):
    shape = (2, 130, 515)
    C, H, W = shape
    orig, recon, body, want = ref_body(shape, lambda: random_planes(np.random.default_rng(sum(shape)), C, H, W), 1)
    x0, y0, w, h = RECTS[name]
    crop = np.ascontiguousarray(recon[:, y0:y0 + h, x0:x0 + w])
    rc, status, rec = gpu_decode(dev, body, C, H, W, crop, (x0, y0, w, h), 0xA5)
    assert rc == 0 and status == 0
    assert np.array_equal(rec, want[:, y0:y0 + h, x0:x0 + w])
    # What lies outside the rectangle is untouched: the decoder is handed a buffer of the rectangle's own [C][h][w] samples and
    # nothing else of the tile, so "outside" is the Arena's guard bands around that buffer, checked inside gpu_decode.
    # the blocks the rectangle does not touch, overwritten with 0xFF: the same rectangle
    _, _, _, _, ext = R.parse_tables(body)
    spoiled = bytearray(body)
    untouched = 0
    for (c, by, bx, rows, cols), (off, n) in zip(R.blocks_of(C, H, W), ext):
        if by + rows <= y0 or by >= y0 + h or bx + cols <= x0 or bx >= x0 + w:
            spoiled[off:off + n] = b"\xff" * n
            untouched += 1
    assert untouched > 0 or name == "whole tile"
    rc, status, rec2 = gpu_decode(dev, bytes(spoiled), C, H, W, crop, (x0, y0, w, h), 0x00)
    assert rc == 0 and status == 0 and np.array_equal(rec2, rec)


# ---------------------------------------------------------------- refusals and damage

def test_short_workspace_and_capacity_are_refused_before_anything_is_written(dev):
    import torch
    L = _lib()
    C, H, W = 2, 70, 300
    orig, recon = random_planes(np.random.default_rng(4), C, H, W)
    cap, nws, ndws = L.lbdrn_resid_bound(C, H, W), L.lbdrn_resid_workspace(C, H, W), L.lbdrn_resid_decode_workspace(C, H, W)
    for short_cap, short_ws in ((1, 0), (0, 1)):
        A = Arena(dev)
        o, r = A.const(orig), A.const(recon)
        body, nb, ws = A.buf(cap, 0xA5, name="body"), A.buf(8, 0xA5, name="body_bytes"), A.buf(nws, 0xA5, name="workspace")
        rc = L.lbdrn_resid_encode(o.ptr, r.ptr, C, H, W, 1, body.ptr, cap - short_cap, nb.ptr, ws.ptr, nws - short_ws, _stream(dev))
        torch.cuda.synchronize()
        assert rc == E_WORKSPACE and L.lbdrn_resid_last_error()
        A.check()
        for b in (body, nb, ws):
            assert bool((b.t == 0xA5).all()), f"{b.name} was written by a refused call"
    good, _ = R.encode_body(orig, recon, 1)
    A = Arena(dev)
    b = A.const(np.frombuffer(good, np.uint8))
    rec, st, ws = A.buf(recon.nbytes, 0xA5).write(recon), A.buf(4, 0xA5, name="status"), A.buf(ndws, 0xA5, name="workspace")
    rc = L.lbdrn_resid_decode(b.ptr, len(good), C, H, W, 0, 0, W, H, rec.ptr, st.ptr, ws.ptr, ndws - 1, _stream(dev))
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE
    A.check()
    assert np.array_equal(rec.numpy(np.uint16).reshape(recon.shape), recon) and bool((st.t == 0xA5).all()) and bool((ws.t == 0xA5).all())
    for rect in ((0, 0, W + 1, H), (-1, 0, 2, 2), (0, 0, 0, 1), (W - 1, H - 1, 2, 1)):      # rectangles outside the tile
        rc = L.lbdrn_resid_decode(b.ptr, len(good), C, H, W, *rect, rec.ptr, st.ptr, ws.ptr, ndws, _stream(dev))
        assert rc == E_ARG
    A.check()


def test_truncated_and_corrupted_bodies_end_in_a_status_or_a_raster(dev):
    C, H, W = 2, 70, 300
    rng = np.random.default_rng(6)
    orig, recon = random_planes(rng, C, H, W)
    good, want = R.encode_body(orig, recon, 1)
    table_end = 20 + 4 * 8
    flagged = refused = passed = 0
    cases = [good[:int(n)] for n in list(rng.integers(0, len(good), 46)) + [1, 19, 20, table_end - 1]]      # 50 truncations
    for t in range(100):
        bad = bytearray(good)
        where = int(rng.integers(0, table_end + 2 * 64)) if t % 2 else int(rng.integers(0, len(good)))
        bad[where] ^= 1 << int(rng.integers(0, 8))
        if t % 5 == 0:
            bad[int(rng.integers(0, len(good)))] = 0xFF
        cases.append(bytes(bad))
    for body in cases:
        if not body:
            continue
        rc, status, rec = gpu_decode(dev, body, C, H, W, recon, (0, 0, W, H), 0xA5)       # (the guards are checked inside)
        if rc != 0:
            refused += 1
            assert rc == E_ARG and np.array_equal(rec, recon)
        elif status:
            flagged += 1
        else:
            passed += 1
    assert flagged > 50 and refused > 0, (flagged, refused, passed)


# ---------------------------------------------------------------- end to end

@contextlib.contextmanager
def _settings(consts=None, base_codec=None, env=None):
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


def _records(path, key):
    return [m.group(1) for m in re.finditer(rf"{key}: (\S+)", open(path).read())]


def _run(workdir, img, name, flags, consts=None, base_codec=None, env=None, window=(100, 90, 60, 70)):
    """encode.main + decode.main (whole, --no-enhancement, --window, -org) of one configuration -> a dict of the results"""
    import decode
    import encode
    from lbdrn_hip import container, raster_io
    src = str(workdir / f"{name}.npy")
    np.save(src, img)
    out = workdir / name
    with _settings(consts, base_codec, env):
        assert encode.main(["-i", src, "-o", str(out), "-e", "2", "-bs", "8192"] + flags) == 0
        (sub,) = [d for d in out.iterdir() if d.is_dir()]
        binp = str(sub / f"{name}.bin")
        res = {"raw": open(binp, "rb").read(), "encode_log": str(sub / "encode.txt")}
        recon = str(sub / f"{name}_recon.tif")
        assert decode.main(["-i", binp]) == 0
        res["full"] = raster_io.read_raster(recon).reshape(img.shape)
        assert decode.main(["-i", binp, "--no-enhancement"]) == 0
        res["base"] = raster_io.read_raster(recon).reshape(img.shape)
        x0, y0, w, h = window
        wout = str(workdir / f"{name}_window.tif")
        assert decode.main(["-i", binp, "--window"] + [str(v) for v in window] + ["-o", wout]) == 0
        res["window"] = raster_io.read_raster(wout).reshape(img.shape[0], h, w)
        assert decode.main(["-i", binp, "-org", src]) == 0
        res["decode_log"] = str(sub / "decode.txt")
    res["trailer"] = container.unpack_residual_trailer(res["raw"])
    return res


@pytest.fixture(scope="module")
def plain(golden, dev, tmp_path_factory):
    """the runs made WITHOUT --max-error, per split ratio: what --no-enhancement must reproduce"""
    img = golden["rasters_learn_bands4"]["img"]
    work = tmp_path_factory.mktemp("resid_plain")
    return {sr: _run(work, img, f"plain{sr}", ["-sr", str(sr)]) for sr in (1, 2)}


@pytest.mark.parametrize("sr", [1, 2])
@pytest.mark.parametrize("T", [0, 2])
def test_encode_decode_end_to_end(golden, dev, tmp_path, plain, T, sr):
    from lbdrn_hip import container
    img = golden["rasters_learn_bands4"]["img"]
    assert img.shape == (4, 256, 256)
    res = _run(tmp_path, img, "scene", ["-sr", str(sr), "--max-error", str(T)])
    err = int(np.abs(res["full"].astype(np.int64) - img).max())
    assert err <= T and (T or np.array_equal(res["full"], img))
    logged = _records(res["encode_log"], "Max error")
    assert len(logged) == sr * sr and max(int(v) for v in logged) == err
    assert _records(res["decode_log"], "Max error") == [str(err)]
    assert len(_records(res["encode_log"], "Residual layer")) == sr * sr
    # the base reconstruction, and the file in front of the trailer, are those of the run without the flag
    base = plain[sr]
    assert np.array_equal(res["base"], base["full"]) and np.array_equal(base["base"], base["full"])
    off = container.residual_trailer_offset(res["raw"])
    assert res["raw"][:off] == base["raw"] and len(base["raw"]) == container.residual_trailer_offset(base["raw"])
    assert base["trailer"] is None and res["trailer"][0] == T and len(res["trailer"][1]) == sr * sr
    x0, y0, w, h = 100, 90, 60, 70          # straddles the four tiles at -sr 2
    assert np.array_equal(res["window"], res["full"][:, y0:y0 + h, x0:x0 + w])
    assert np.array_equal(base["window"], base["full"][:, y0:y0 + h, x0:x0 + w])


@pytest.mark.parametrize("name,flags,consts,codec,env", [
    ("jp2gpu", ["-sr", "2", "-bs", "512"], {}, "jp2-gpu", {"LBDRN_BASE_DECODER": "gpu"}),
    ("relu", ["-sr", "2", "-bs", "512"], {"HIDDEN_ACTIVATION": "relu"}, None, {}),
])
def test_other_payloads_and_the_relu_header(golden, dev, tmp_path, name, flags, consts, codec, env):
    from lbdrn_hip import container
    img = np.ascontiguousarray(golden["rasters_learn_bands4"]["img"][:, :96, :80])
    res = _run(tmp_path, img, name, flags + ["--max-error", "0"], consts, codec, env, window=(30, 40, 20, 16))
    assert np.array_equal(res["full"], img)
    assert np.array_equal(res["window"], img[:, 40:56, 30:50])
    assert not np.array_equal(res["base"], img)
    assert container.header_activation(res["raw"]) == ("relu" if name == "relu" else None)


def test_fit_on_the_generic_path_decodes_within_the_bound_on_the_mfma_path(golden, dev):
    """the closed loop's premise: the reconstruction the encoder codes against is the one every path computes"""
    import torch
    from lbdrn_hip import codec, container, ops
    from lbdrn_hip.features import FeatCfg
    img = golden["rasters_learn_bands4"]["img"]
    K, D, bc, nl, cfg = 5, 2, 64, 2, FeatCfg()
    torch.manual_seed(19920517)
    fit = codec.fit_device(ops.to_device_u16(img, dev), K, D, bc, nl, 1e-3, 8192, 2, cfg=cfg, path=ops._lib.PATH_GENERIC)
    res = codec._host_result(fit, 2, {}, False)
    nn = container.encode_weights(res.params, 16)
    for tau in (0, 2):
        body, err = codec.residual_encode(res, tau, img, nn, K, D, bc, nl, cfg=cfg, device=dev, path=ops._lib.PATH_GENERIC)
        params = torch.from_numpy(container.decode_weights(nn)).to(dev)
        rec = ops.decode_fused(fit.geom, fit.net, fit.msb, params, path=ops._lib.PATH_MFMA).contiguous()
        out = ops.from_device_u16(codec.residual_apply(body, rec))
        assert int(np.abs(out.astype(np.int64) - img).max()) == err <= tau


def test_tiles_alone_and_four_in_flight_give_identical_bodies(golden, dev):
    import torch
    from lbdrn_hip import codec, container, ops
    from lbdrn_hip.features import FeatCfg
    img = golden["rasters_learn_bands4"]["img"]
    tiles = [np.ascontiguousarray(img[:, y:y + 128, x:x + 128]) for y in (0, 128) for x in (0, 128)]
    K, D, bc, nl, cfg = 5, 2, 64, 2, FeatCfg()
    bodies = {}
    for in_flight in (1, 4):
        torch.manual_seed(19920517)
        draws = [codec.draw_fit(cfg.feature_dim(4, D), bc, 4, nl, 2, 1) for _ in tiles]
        results = codec.fit_images(tiles, K, D, bc, nl, 1e-3, 8192, 2, cfg=cfg, device=dev, host_msb=False, draws=draws, in_flight=in_flight)
        bodies[in_flight] = [codec.residual_encode(r, 1, t, container.encode_weights(r.params, 16), K, D, bc, nl, cfg=cfg, device=dev)[0]
                             for r, t in zip(results, tiles)]
    assert bodies[1] == bodies[4] and len(set(bodies[1])) == 4
