"""Host side of the windowed decode (codec.decode_window, decode.py --window): which tiles a window touches and where its
pieces go, the margin around a piece, the positional tables of a crop, the errors, and the command line around it.  The
kernels are not under test here (tests/test_gpu_window_decode.py): where a decoded piece is needed a stand-in supplies
it."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

SIZES = ((50, 37), (37, 50), (48, 48), (7, 5))


def _owner(width, height, sr):
    """Brute force: the tile index of every scene pixel."""
    from LBDRNdataset import tile_windows
    own = np.full((height, width), -1, np.int64)
    for t, (_, _, x0, y0, w, h) in enumerate(tile_windows(width, height, sr)):
        assert (own[y0:y0 + h, x0:x0 + w] == -1).all()
        own[y0:y0 + h, x0:x0 + w] = t
    assert (own >= 0).all()
    return own


def _windows(width, height, rng, n=40):
    yield 0, 0, width, height
    for x, y in ((0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, height // 2)):
        yield x, y, 1, 1
    for _ in range(n):
        x0, y0 = int(rng.integers(0, width)), int(rng.integers(0, height))
        yield x0, y0, int(rng.integers(1, width - x0 + 1)), int(rng.integers(1, height - y0 + 1))


@pytest.mark.parametrize("sr", (1, 2, 3))
def test_tile_selection_and_clipping_against_a_brute_force_mask(sr):
    from lbdrn_hip import codec
    from LBDRNdataset import tile_windows
    rng = np.random.default_rng(sr)
    for width, height in SIZES:
        own = _owner(width, height, sr)
        tiles = list(tile_windows(width, height, sr))
        for win in _windows(width, height, rng):
            x0, y0, w, h = win
            want = own[y0:y0 + h, x0:x0 + w]
            pieces = codec.window_pieces(width, height, sr, win, 2)
            assert [p.tile for p in pieces] == sorted(set(want.ravel().tolist())), (width, height, win)
            got = np.full((h, w), -1, np.int64)
            for p in pieces:
                assert (p.tx, p.ty, p.tw, p.th) == tiles[p.tile][2:]
                assert 0 <= p.xa < p.xb <= p.tw and 0 <= p.ya < p.yb <= p.th
                assert (p.ox, p.oy) == (p.tx + p.xa - x0, p.ty + p.ya - y0)
                assert (got[p.oy:p.oy + p.yb - p.ya, p.ox:p.ox + p.xb - p.xa] == -1).all()      # no pixel twice
                got[p.oy:p.oy + p.yb - p.ya, p.ox:p.ox + p.xb - p.xa] = p.tile
            assert np.array_equal(got, want), (width, height, win)                               # every pixel, from its own tile


def test_margin_is_D_clipped_to_the_tile_edges():
    from lbdrn_hip import codec
    # one 20 x 16 tile, D = 3: distances D-1, D, D+1 from each edge
    for D in (0, 1, 2, 3):
        for gap in (0, max(D - 1, 0), D, D + 1):
            (p,) = codec.window_pieces(20, 16, 1, (gap, gap, 20 - 2 * gap, 16 - 2 * gap), D)
            assert (p.left, p.right, p.top, p.bottom) == (min(D, gap),) * 4
            (p,) = codec.window_pieces(20, 16, 1, (gap, 5, 2, 3), D)
            assert (p.left, p.right, p.top, p.bottom) == (min(D, gap), min(D, 20 - gap - 2), min(D, 5), min(D, 16 - 8))
    # the margin stops at the TILE's edge, not at the scene's: tiles of 50 x 37 at -sr 3 are 16 (18) x 12 (13)
    pieces = codec.window_pieces(50, 37, 3, (15, 11, 3, 3), 2)
    assert [p.tile for p in pieces] == [0, 1, 3, 4]
    assert [(p.left, p.right, p.top, p.bottom) for p in pieces] == [(2, 0, 2, 0), (0, 2, 2, 0), (2, 0, 0, 2), (0, 2, 0, 2)]


@pytest.mark.parametrize("D", (0, 1, 2, 3))
def test_a_crop_with_its_margin_sees_the_neighbourhoods_of_the_whole_tile(D):
    """A host model of what the apply kernels compute -- any per-pixel function of the reflect-padded (2D+1)^2
    neighbourhood (ref LBDRNdataset.py:120-125) -- on the crop with its margin gives the whole tile's values inside."""
    from lbdrn_hip import codec
    rng = np.random.default_rng(D)
    weights = rng.standard_normal((2 * D + 1, 2 * D + 1))

    def model(plane):
        pad = np.pad(plane.astype(np.float64), D, mode="reflect")
        return (np.lib.stride_tricks.sliding_window_view(pad, weights.shape) * weights).sum(axis=(2, 3))

    for width, height, sr in ((50, 37, 3), (23, 19, 2), (17, 11, 1)):
        scene = rng.integers(0, 2000, (height, width))
        full = np.zeros((height, width))
        from LBDRNdataset import tile_windows
        for _, _, x0, y0, w, h in tile_windows(width, height, sr):
            full[y0:y0 + h, x0:x0 + w] = model(scene[y0:y0 + h, x0:x0 + w])
        for win in _windows(width, height, rng, 25):
            x0, y0, w, h = win
            out = np.full((h, w), np.nan)
            for p in codec.window_pieces(width, height, sr, win, D):
                tile = scene[p.ty:p.ty + p.th, p.tx:p.tx + p.tw]
                rec = model(tile[p.ya - p.top:p.yb + p.bottom, p.xa - p.left:p.xb + p.right])
                out[p.oy:p.oy + p.yb - p.ya, p.ox:p.ox + p.xb - p.xa] = rec[p.top:p.top + p.yb - p.ya, p.left:p.left + p.xb - p.xa]
            assert np.array_equal(out, full[y0:y0 + h, x0:x0 + w]), (width, height, sr, win)


@pytest.mark.parametrize("embedding", (False, True))
def test_table_slices_keep_each_pixels_tile_coordinate(embedding):
    from lbdrn_hip.features import FeatCfg, pos_tables, window_tables
    cfg = FeatCfg(use_coordinates=True, embedding=embedding)
    H, W = 24, 20
    rowtab, coltab = pos_tables(H, W, cfg)
    for rows, cols in (((0, H), (0, W)), ((5, 9), (3, 4)), ((H - 1, H), (W - 3, W)), ((0, 1), (0, 1))):
        r, c = window_tables(H, W, cfg, rows, cols)
        assert r.shape == (rows[1] - rows[0], cfg.P) and c.shape == (cols[1] - cols[0], cfg.P)
        assert r.flags.c_contiguous and c.flags.c_contiguous and r.dtype == np.float32
        for i in range(r.shape[0]):
            assert np.array_equal(r[i].view(np.uint32), rowtab[rows[0] + i].view(np.uint32))
        for j in range(c.shape[0]):
            assert np.array_equal(c[j].view(np.uint32), coltab[cols[0] + j].view(np.uint32))
    # the crop's own tables are another function: a ramp over the crop, not over the tile
    r, c = window_tables(H, W, cfg, (5, 9), (3, 8))
    own_r, own_c = pos_tables(4, 5, cfg)
    assert not np.array_equal(r, own_r) and not np.array_equal(c, own_c)
    # without coordinates there is nothing to slice
    r, c = window_tables(H, W, FeatCfg(), (5, 9), (3, 8))
    assert r.shape == (4, 0) and c.shape == (5, 0)


def test_geometry_refuses_tables_of_another_size():
    from lbdrn_hip import ops
    from lbdrn_hip.features import FeatCfg, window_tables
    cfg = FeatCfg(use_coordinates=True)
    with pytest.raises(ValueError, match="positional tables"):
        ops.FeatureGeometry(2, 4, 6, 5, 1, 100, cfg, "cpu", tables=window_tables(24, 20, cfg, (5, 9), (3, 8)))


def _header_only(width, height, sr=1):
    from lbdrn_hip import container
    return container.pack_header(sr, width, height, 5, 64, 2, 2, [0] * sr * sr, [0] * sr * sr)


@pytest.mark.parametrize("window", ((0, 0, 0, 5), (0, 0, 5, 0), (3, 3, -1, 2), (-1, 0, 4, 4), (0, -1, 4, 4), (47, 0, 4, 4),
                                    (0, 30, 4, 8), (50, 0, 1, 1), (0, 37, 1, 1), (0, 0, 51, 37), (0, 0, 50, 38)))
def test_empty_and_out_of_range_windows_are_value_errors_that_name_the_scene(window, monkeypatch):
    from lbdrn_hip import codec, container, ops

    def no_device_work(*a, **k):
        raise AssertionError("device work before the window was checked")
    monkeypatch.setattr(container, "decode_base", no_device_work)
    monkeypatch.setattr(ops, "decode_fused", no_device_work)
    with pytest.raises(ValueError, match="50 x 37"):
        codec.check_window(window, 50, 37)
    with pytest.raises(ValueError, match="50 x 37"):
        codec.window_pieces(50, 37, 3, window, 2)
    with pytest.raises(ValueError, match="50 x 37"):
        codec.decode_window(_header_only(50, 37, 3), window)
    with pytest.raises(ValueError, match="four integers"):
        codec.check_window((1, 2, 3), 50, 37)
    assert codec.check_window((49, 36, 1, 1), 50, 37) == (49, 36, 1, 1)
    assert codec.check_window(np.array([0, 0, 50, 37]), 50, 37) == (0, 0, 50, 37)


# ---------------------------------------------------------------- the command line

SCENE = np.random.default_rng(7).integers(0, 4000, (2, 8, 12)).astype(np.uint16)


def _stub_pieces(bitstream, window, device="cuda:0", path=0, cfg=None, take=None):
    """Stands where codec.decode_window_pieces stands (the GPU work): the pieces of SCENE + 1."""
    from lbdrn_hip import codec, container
    _, sr, width, height, K, bc, nl, D, _, _ = container.unpack_header(bitstream)
    out = []
    for k, p in enumerate(codec.window_pieces(width, height, sr, window, D)):
        if take is None or take(k, p):
            rec = (SCENE + 1)[:, p.ty + p.ya:p.ty + p.yb, p.tx + p.xa:p.tx + p.xb]
            out.append((p, torch.from_numpy(np.ascontiguousarray(rec).view(np.int16))))
    return (width, height), out


def _records(path):
    with open(path) as f:
        return [re.sub(r"^\[[^\]]*\] ", "", line.rstrip("\n")) for line in f]


def _blob():
    from lbdrn_hip import container
    nn, base = [b"w" * 10] * 4, [bytes(range(t, t + 48)) + b"pad" * t for t in range(4)]
    blob = container.pack_header(2, 12, 8, 3, 64, 2, 2, [len(x) for x in nn], [len(x) for x in base])
    for x, y in zip(nn, base):
        blob += x + y
    return blob


def test_window_flag_parses_and_leaves_the_plain_decode_alone(tmp_path, monkeypatch):
    import decode
    from lbdrn_hip import codec, container
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    (tmp_path / "img.bin").write_bytes(_blob())
    binp = str(tmp_path / "img.bin")
    org = str(tmp_path / "org.npy")
    np.save(org, SCENE)
    seen = []
    monkeypatch.setattr(decode, "decode_window_main", lambda args, rank, world: seen.append(args) or 0)
    assert decode.main(["-i", binp, "--window", "3", "2", "5", "4"]) == 0
    assert seen[-1].window == [3, 2, 5, 4] and seen[-1].out_path is None and seen[-1].org_path is None
    assert decode.main(["-i", binp, "--window", "0", "0", "1", "1", "-o", "x.tif", "-org", org]) == 0
    assert (seen[-1].window, seen[-1].out_path, seen[-1].org_path) == ([0, 0, 1, 1], "x.tif", org)
    for bad in (["--window", "1", "2", "3"], ["--window", "a", "0", "1", "1"], ["-o", "x.tif"]):
        with pytest.raises(SystemExit):
            decode.main(["-i", binp] + bad)
    assert sorted(os.listdir(tmp_path)) == ["img.bin", "org.npy"]
    # without the flag: the whole decode as ever -- decode.txt with its records, the raster removed after -org, and a second
    # run that stops at the marker; the window path is never entered
    n_seen = len(seen)
    monkeypatch.setattr(codec, "apply_image", lambda base, params, K, D, bc, nl, cfg=None, device=None, **kw:
                        (np.asarray(base).astype(np.uint16) << K) + 1)
    monkeypatch.setattr(container, "decode_weights", lambda payload, expected=None: np.zeros(4, np.float32))
    monkeypatch.setattr(container, "decode_base", lambda payload, device=None, keep_on_device=False:
                        np.frombuffer(payload[:48], np.uint8).reshape(2, 4, 6).copy())
    assert decode.main(["-i", binp, "-org", org]) == 0
    recs = _records(tmp_path / "decode.txt")
    assert [r.split(":")[0] for r in recs] == ["Binstream", "Time elapsed", "MSE", "PSNR", "Total size"]
    assert sorted(os.listdir(tmp_path)) == ["decode.txt", "img.bin", "org.npy"]
    assert decode.main(["-i", binp, "-org", org]) == 0 and _records(tmp_path / "decode.txt") == recs
    assert len(seen) == n_seen


def test_window_cli_writes_the_crop_and_never_touches_the_marker(tmp_path, monkeypatch, capsys):
    import decode
    from lbdrn_hip import codec, raster_io
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(codec, "decode_window_pieces", _stub_pieces)
    (tmp_path / "img.bin").write_bytes(_blob())
    binp = str(tmp_path / "img.bin")
    org = str(tmp_path / "org.npy")
    np.save(org, SCENE)
    marker = tmp_path / "decode.txt"
    marker.write_text("[t] Total size: 1 bytes, bpsp=0.5\n")          # "already decoded": the window decode runs anyway
    assert decode.main(["-i", binp, "--window", "4", "2", "5", "4", "-org", org]) == 0
    assert marker.read_text() == "[t] Total size: 1 bytes, bpsp=0.5\n"
    rec = raster_io.read_raster(str(tmp_path / "img_recon_x4_y2_w5_h4.tif"))
    assert rec.dtype == np.uint16 and np.array_equal(rec, (SCENE + 1)[:, 2:6, 4:9])      # (crosses all four tiles)
    recs = _records(tmp_path / "decode_window.txt")
    assert [r.split(":")[0] for r in recs] == ["Binstream", "Window", "Recon", "Time elapsed", "MSE", "PSNR"]
    assert recs[1] == "Window: x0=4 y0=2 w=5 h=4 of 12 x 8" and not any("bpsp" in r for r in recs)
    assert float(recs[4].split(": ")[1]) == 1.0 and "Window: x0=4" in capsys.readouterr().out
    out = str(tmp_path / "sub.npy")
    assert decode.main(["-i", binp, "--window", "11", "7", "1", "1", "-o", out]) == 0
    assert np.array_equal(np.load(out), (SCENE + 1)[:, 7:8, 11:12])
    with pytest.raises(ValueError, match="12 x 8"):
        decode.main(["-i", binp, "--window", "8", "0", "5", "1"])
    assert marker.read_text() == "[t] Total size: 1 bytes, bpsp=0.5\n"


def _window_worker(rank, world, port, bin_path, org):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import decode
    from lbdrn_hip import codec
    dealt = []

    def pieces(bitstream, window, device="cuda:0", path=0, cfg=None, take=None):
        size, out = _stub_pieces(bitstream, window, device, path, cfg, take)
        dealt.extend(p.tile for p, _ in out)
        return size, out
    codec.decode_window_pieces = pieces
    assert decode.main(["-i", bin_path, "--window", "1", "3", "11", "4", "-org", org]) == 0
    assert dealt == [[0, 2], [1, 3]][rank]          # the touched tiles, dealt like all tiles of a whole decode


def test_window_cli_deals_the_touched_tiles_over_the_ranks(tmp_path):
    import torch.multiprocessing as mp
    from lbdrn_hip import raster_io
    (tmp_path / "img.bin").write_bytes(_blob())
    org = str(tmp_path / "org.npy")
    np.save(org, SCENE)
    mp.spawn(_window_worker, args=(2, 29700 + os.getpid() % 200, str(tmp_path / "img.bin"), org), nprocs=2, join=True)
    rec = raster_io.read_raster(str(tmp_path / "img_recon_x1_y3_w11_h4.tif"))
    assert np.array_equal(rec, (SCENE + 1)[:, 3:7, 1:12])
    recs = _records(tmp_path / "decode_window.txt")
    assert [r.split(":")[0] for r in recs] == ["Binstream", "Window", "Recon", "Time elapsed", "MSE", "PSNR"]


@pytest.mark.parametrize("sr,D", ((1, 2), (2, 1), (3, 3)))
def test_decode_window_around_the_oracle_equals_the_crop_of_the_whole_decode(sr, D, monkeypatch):
    """codec.decode_window with the CPU oracle standing where the apply kernel stands (ops.decode_fused) and raw planes as
    payloads: tile skip, margin, placement and the tile-wide MSB maximum on the real network arithmetic, bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    from lbdrn_hip import codec, container, ops
    from lbdrn_hip.features import FeatCfg
    from LBDRNdataset import tile_windows
    C, H, W, K, bc, nl = 3, 29, 34, 4, 32, 1
    rng = np.random.default_rng(10 * sr + D)
    msb = rng.integers(0, 200, (C, H, W)).astype(np.uint16)
    msb[:, -1, -1] = 900                                              # the last tile's maximum sits in its corner
    F = C * (2 * D + 1) ** 2
    n_par = ops.param_count(ops.make_net(F, bc, C, nl))
    tiles = list(tile_windows(W, H, sr))
    weights = [(rng.standard_normal(n_par) * 0.3).astype(np.float32) for _ in tiles]
    nn = [w.tobytes() for w in weights]
    base = [np.ascontiguousarray(msb[:, y0:y0 + h, x0:x0 + w]).tobytes() + bytes([h, w]) for _, _, x0, y0, w, h in tiles]
    blob = container.pack_header(sr, W, H, K, bc, nl, D, [len(x) for x in nn], [len(x) for x in base])
    for x, y in zip(nn, base):
        blob += x + y
    monkeypatch.setattr(container, "decode_weights", lambda buf, expected=None: np.frombuffer(buf, np.float32))
    monkeypatch.setattr(container, "decode_base", lambda buf, device=None, keep_on_device=False:
                        np.frombuffer(buf[:-2], np.uint16).reshape(C, buf[-2], buf[-1]))

    def oracle_apply(geom, net, plane, params, want_y=False, path=0, ws=None):
        rec = O.decode(plane.numpy().view(np.uint16), geom.K, geom.D, O.FeatCfg(), params.numpy(), net.bc, net.nl, geom.msb_max)
        return torch.from_numpy(np.ascontiguousarray(rec).view(np.int16))
    monkeypatch.setattr(ops, "decode_fused", oracle_apply)
    full = np.zeros((C, H, W), np.uint16)
    for (_, _, x0, y0, w, h), p in zip(tiles, weights):
        t = msb[:, y0:y0 + h, x0:x0 + w]
        full[:, y0:y0 + h, x0:x0 + w] = O.decode(np.ascontiguousarray(t), K, D, O.FeatCfg(), p, bc, nl, int(t.max()))
    for win in _windows(W, H, rng, 12):
        x0, y0, w, h = win
        got = codec.decode_window(blob, win, device="cpu", cfg=FeatCfg(), keep_on_device=False)
        assert got.dtype == np.uint16 and np.array_equal(got, full[:, y0:y0 + h, x0:x0 + w]), win
