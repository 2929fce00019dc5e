"""encode.py --nodata V --nodata-fit valid on the GPU.

The masked ranking sum (LBDRN_EVAL_VALID, lbdrn_hip.h): every serving leg of lbdrn_eval_sse at K = 5, D = 2 on 4 x 30 x 41 (one
ragged tile row, one tile column) and 8 x 48 x 130 (three tile columns, the last ragged), the instance confirmed through
lbdrn_apply_instance, against four masks -- a corner collar of V = 0 with void pixels, a V that some bands of a pixel hold and
others do not, a V that occurs nowhere, a raster of nothing but V.

  canonical legs   y comes from lbdrn_decode_fused(y_out=...), the same canonical sigmoid, bit-exact by the existing tests; each
                   kept term is formed in numpy float32 exactly as the kernel forms it and the terms are added with math.fsum.
                   The kernel's double sum of n non-negative terms may differ from the exact one by at most n 2^-53 relative:
                   the bound of ANY order of double additions, derived and not tuned.
  fast, x16 legs   within 1e-6 relative of the canonical masked sum: what lbdrn_hip.h states for these flags.

The fit (codec.fit_device / fit_group / fit_many with nodata=): bc = 64, two hidden layers (the fused step) on 4 x 64 x 96 with a
triangular collar, batch size 256, 3 epochs, against the chain spelled out here -- valid_idx[randperm] through ops.train_epoch,
ops.eval_sse(nodata=V), the reference's best-epoch rule -- bit for bit.  Then the command lines end to end."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from guarded import FILLS, Arena  # noqa: E402
from lbdrn_hip import _lib, codec, ops, sampler  # noqa: E402
from lbdrn_hip.features import FeatCfg  # noqa: E402
from lbdrn_hip.synth import synthetic_tile  # noqa: E402
from test_gpu_fuzz import _params  # noqa: E402
from test_gpu_window_decode import _records, _settings  # noqa: E402

pytestmark = pytest.mark.gpu
GEN, MFMA = _lib.PATH_GENERIC, _lib.PATH_MFMA
FAST, X16, BACKGROUND, VALID = _lib.EVAL_FAST, _lib.EVAL_X16, _lib.EVAL_BACKGROUND, _lib.EVAL_VALID
K, D, NL = 5, 2, 2
SHAPES = ((4, 30, 41), (8, 48, 130))
# leg -> (path, bc, activation, flags, (family, NT, relu | NL, serving mode) of lbdrn_apply_instance, the leg its sum is held to)
LEGS = {
    "mfma_bc32": (MFMA, 32, ops.ACT_SINE, 0, (1, 1, 0, 1), None),
    "mfma_bc64": (MFMA, 64, ops.ACT_SINE, 0, (1, 2, 0, 1), None),
    "fast_bc64": (MFMA, 64, ops.ACT_SINE, FAST, (1, 2, 0, 2), "mfma_bc64"),
    "x16_bc64": (MFMA, 64, ops.ACT_SINE, FAST | X16, (1, 2, 0, 3), "mfma_bc64"),
    "relu_bc64": (MFMA, 64, ops.ACT_RELU, 0, (1, 2, 1, 1), None),
    "wide_bc256": (MFMA, 256, ops.ACT_SINE, 0, (2, 16, 2, 1), None),
    "wide_fast_bc256": (MFMA, 256, ops.ACT_SINE, FAST, (2, 16, 2, 2), "wide_bc256"),
    "generic_bc64": (GEN, 64, ops.ACT_SINE, 0, None, None),
}


def _bits(x):
    return np.float64(x).tobytes()


def _masks(shape):
    """name -> (image, V)"""
    C, H, W = shape
    base = synthetic_tile(7 + C, C, H, W).astype(np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    collar = np.where(base == 0, 1, base).astype(np.uint16)
    collar[:, yy + xx < H // 2 + 5] = 0                       # void pixels: every band
    partial = np.where(base == 1000, 1001, base).astype(np.uint16)
    partial[0, 5:20, 3:30] = 1000                             # some bands of a pixel only: no pixel of it is void
    partial[C - 1, 10:25, 20:W] = 1000
    absent = int(np.setdiff1d(np.arange(1, 4096), base)[0])
    assert (collar == 0).all(0).sum() > 100 and not (partial == 1000).all(0).any() and (partial == 1000).any(0).sum() > 400
    return {"collar": (collar, 0), "partial": (partial, 1000), "nowhere": (base, absent), "all": (np.full(shape, 1000, np.uint16), 1000)}


_INPUTS = {}


def _inputs(dev, shape, mask):
    """(image, V, image / MSB plane in HBM, MSB maximum) of one shape and mask, made once"""
    if (shape, mask) not in _INPUTS:
        img, V = _masks(shape)[mask]
        img_d = ops.to_device_u16(img, dev)
        msb_d, mx = ops.split_bits(img_d, K)
        _INPUTS[(shape, mask)] = (img, V, img_d, msb_d, mx)
    return _INPUTS[(shape, mask)]


def _net(leg, shape, dev):
    path, bc, act, flags, instance, _ = LEGS[leg]
    C = shape[0]
    F = FeatCfg().feature_dim(C, D)
    p = torch.from_numpy(_params(np.random.default_rng(bc + C), F, bc, C, NL, 2.5)).to(dev)
    return ops.make_net(F, bc, C, NL, act), p


def _sse(dev, leg, shape, mask, valid=True, background=False):
    path, bc, act, flags, _, _ = LEGS[leg]
    img, V, img_d, msb_d, mx = _inputs(dev, shape, mask)
    net, p = _net(leg, shape, dev)
    geom = ops.FeatureGeometry(*shape, K, D, mx, FeatCfg(), dev)
    sse = ops.eval_sse(geom, net, img_d, msb_d, p, path, background=background, fast=bool(flags & FAST), x16=bool(flags & X16),
                       nodata=V if valid else None)
    return float(sse.item())


_EXACT = {}


def _exact_masked_sum(dev, leg, shape, mask):
    """(math.fsum of the kept terms, their number) from the decode pass's sigmoid outputs, in the kernel's float32 arithmetic"""
    key = (leg, shape, mask)
    if key not in _EXACT:
        path = LEGS[leg][0]
        img, V, img_d, msb_d, mx = _inputs(dev, shape, mask)
        net, p = _net(leg, shape, dev)
        geom = ops.FeatureGeometry(*shape, K, D, mx, FeatCfg(), dev)
        _, y = ops.decode_fused(geom, net, msb_d, p, want_y=True, path=path)
        y = y.cpu().numpy().astype(np.float32)                                       # [H W][C]
        samples = img.reshape(shape[0], -1).T                                         # [H W][C]
        lab = (samples & ((1 << K) - 1)).astype(np.float32) / np.float32((1 << K) - 1)
        d = y - lab
        terms = (d * d)[samples != V]
        assert terms.dtype == np.float32
        _EXACT[key] = (math.fsum(terms.astype(np.float64).tolist()), int(terms.size))
    return _EXACT[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("leg", list(LEGS))
def test_masked_sum(dev, leg, shape):
    path, bc, act, flags, instance, held_to = LEGS[leg]
    C, H, W = shape
    if instance is not None:      # the intended instance serves the case, with the flag and without it, whatever the mask
        for mask in ("collar", "partial", "nowhere", "all"):
            mx = _inputs(dev, shape, mask)[4]
            geom = ops.FeatureGeometry(*shape, K, D, mx, FeatCfg(), dev)
            net, _ = _net(leg, shape, dev)
            for word in (flags, flags | VALID):
                out = (ctypes.c_int32 * 8)()
                assert _lib.lib().lbdrn_apply_instance(ctypes.byref(geom.c), ctypes.byref(net), MFMA | word, out) == 0
                assert tuple(out[:4]) == instance and out[7] == -(-W // 64) * -(-H // out[4]) > 1, (mask, list(out))
                assert out[6] == int(bool(flags & X16))
    # 1. V nowhere in the image: the flagless sum, bit for bit
    assert _bits(_sse(dev, leg, shape, "nowhere")) == _bits(_sse(dev, leg, shape, "nowhere", valid=False))
    # 2. nothing but V: exactly 0.0 (and the flagless sum of that raster is not)
    assert _bits(_sse(dev, leg, shape, "all")) == _bits(0.0) and _sse(dev, leg, shape, "all", valid=False) > 0.0
    for mask in ("collar", "partial", "nowhere"):
        got = _sse(dev, leg, shape, mask)
        if held_to is None:
            # 3. canonical: the exact sum of the kept float32 terms, to the bound of a double summation
            want, n = _exact_masked_sum(dev, leg, shape, mask)
            img, V = _inputs(dev, shape, mask)[:2]
            assert n == int((img != V).sum()) and (mask == "nowhere") == (n == C * H * W)
            print(f"{leg} {shape} {mask}: kernel {got!r} exact {want!r} |diff|/exact {abs(got - want) / want:.3e} bound {n * 2.0 ** -53:.3e}")
            assert abs(got - want) <= n * 2.0 ** -53 * want, (got, want, n)
        else:
            # 4. fast / x16: within 1e-6 relative of the canonical masked sum
            canon = _sse(dev, held_to, shape, mask)
            print(f"{leg} {shape} {mask}: {got!r} canonical {canon!r} rel {abs(got - canon) / canon:.3e}")
            assert abs(got - canon) <= 1e-6 * canon, (got, canon)
        if mask != "nowhere":
            assert got < _sse(dev, leg, shape, mask, valid=False)      # the mask left something out
        # 5. the same bits on half as many workgroups, on a second stream, and again
        again = _sse(dev, leg, shape, mask)
        back = _sse(dev, leg, shape, mask, background=True)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            other = _sse(dev, leg, shape, mask, background=True)
        torch.cuda.current_stream(dev).wait_stream(side)
        assert _bits(got) == _bits(again) == _bits(back) == _bits(other), (got, again, back, other)


@pytest.mark.parametrize("leg", list(LEGS))
def test_masked_sum_bad_field_and_buffer_hygiene(dev, leg):
    path, bc, act, flags, _, _ = LEGS[leg]
    shape = SHAPES[0]
    img, V, img_d, msb_d, mx = _inputs(dev, shape, "collar")
    msb_np = (img >> K).astype(np.uint16)
    net, p = _net(leg, shape, dev)
    lib = _lib.lib()

    def run(fill, reserved, word):
        A = Arena(dev)
        geom = ops.FeatureGeometry(*shape, K, D, mx, FeatCfg(), dev)
        g = _lib.Geom.from_buffer_copy(geom.c)
        g.reserved = reserved
        src, msb, par = A.const(img, "img"), A.const(msb_np, "msb"), A.const(p.cpu().numpy(), "params")
        sse = A.buf(8, fill, name="sse")
        nws = lib.lbdrn_apply_workspace(ctypes.byref(g), ctypes.byref(net))
        assert nws == lib.lbdrn_apply_workspace(ctypes.byref(geom.c), ctypes.byref(net))      # the field sizes nothing
        ws = A.buf(nws, fill, name="workspace")
        with torch.cuda.device(dev):
            rc = lib.lbdrn_eval_sse(ctypes.byref(g), ctypes.byref(net), src.ptr, msb.ptr, par.ptr, sse.ptr, ws.ptr, nws, path | word,
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            torch.cuda.synchronize(dev)
        A.check()
        return rc, sse.numpy(np.float64), ws

    # 6. the field outside 0..65535 with the flag: LBDRN_E_ARG, nothing launched -- *sse and the workspace keep their fill
    for bad in (65536, -1):
        rc, sse, ws = run(0xA5, bad, flags | VALID)
        assert rc == -1 and b"reserved" in lib.lbdrn_last_error()
        assert sse.tobytes() == b"\xA5" * 8 and bool((ws.as_u8() == 0xA5).all())
    # without the flag the field is not read: any value, the flagless sum
    plain = [run(0x00, r, flags) for r in (0, 65536, -7)]
    assert all(rc == 0 for rc, _, _ in plain) and len({s.tobytes() for _, s, _ in plain}) == 1
    assert plain[0][1].tobytes() == _bits(_sse(dev, leg, shape, "collar", valid=False))
    # 7. poisoned workspace and *sse, guards around every buffer: one result, the wrapper's
    outs = [run(fill, V, flags | VALID) for fill in FILLS]
    assert all(rc == 0 for rc, _, _ in outs) and len({s.tobytes() for _, s, _ in outs}) == 1
    assert outs[0][1].tobytes() == _bits(_sse(dev, leg, shape, "collar"))


# ---------------------------------------------------------------- the fit

FIT_SHAPE, BC, BS, EPOCHS, LR = (4, 64, 96), 64, 256, 3, 1e-3


def _tile(kind):
    C, H, W = FIT_SHAPE
    img = synthetic_tile(3, C, H, W).astype(np.uint16)
    img[img == 0] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "collar":
        img[:, 3 * yy + 2 * xx < 150] = 0      # a triangle in the corner
        img[1, 40, 50] = 0                     # one band's sample more: that pixel stays valid
    elif kind == "collar2":
        img[:, 3 * yy + 2 * xx < 100] = 0
    elif kind == "void":
        img[:] = 0
    return img


def _draws(seed=19920517):
    torch.manual_seed(seed)
    F = FeatCfg().feature_dim(FIT_SHAPE[0], D)
    return codec.draw_fit(F, BC, FIT_SHAPE[0], NL, EPOCHS)


def _fit(dev, img, Kf=K, nodata=None, draws=None):
    return codec.fit_device(ops.to_device_u16(img, dev), Kf, D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), keep_losses=True,
                            draws=draws or _draws(), nodata=nodata)


def _same_fit(a, b):
    torch.cuda.synchronize()
    eq = lambda x, y: x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert eq(a.best_params, b.best_params) and eq(a.mse_log, b.mse_log) and eq(a.losses, b.losses)
    assert a.evaluated == b.evaluated and a.msb_max == b.msb_max and torch.equal(a.msb, b.msb)


def test_fit_device_is_the_spelled_out_chain(dev):
    img = _tile("collar")
    C, H, W = FIT_SHAPE
    dr = _draws()
    fit = _fit(dev, img, nodata=0, draws=dr)
    # the chain, step by step
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, FeatCfg(), dev)
    net = ops.make_net(geom.F, BC, C, NL, ops.ACT_SINE)
    valid_idx = torch.from_numpy(np.flatnonzero(~(img == 0).all(0).reshape(-1)).astype(np.int64)).to(dev)
    n = int(valid_idx.numel())
    assert 0 < n < H * W and fit.n_valid == n and n % BS != 0
    steps = -(-n // BS)
    count = int((img != 0).sum())
    assert C * n - count == 1      # the pixel that is nodata in one band only is stepped, its nodata sample is not ranked
    params = dr.params.to(dev, copy=True).contiguous()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    losses = torch.zeros((EPOCHS, steps), dtype=torch.float32, device=dev)
    mse_log = torch.zeros((EPOCHS, 2), dtype=torch.float32, device=dev)
    lrs = codec.lr_schedule(LR, EPOCHS)
    best, best_mse = params.clone(), np.float32(1e6)
    for e in range(1, EPOCHS + 1):
        perm = sampler.permutation(dr.train_seeds[e - 1], n).to(dev)
        ops.train_epoch(geom, net, img_d, msb_d, valid_idx[perm], BS, params, m, v, (e - 1) * steps, lrs[e - 1], losses[e - 1])
        sse = ops.eval_sse(geom, net, img_d, msb_d, params, fast=codec.fast_evaluation(), x16=codec.exact16_evaluation(), nodata=0)
        mse = np.float32(np.float64(sse.item()) / np.float64(count))
        improved = bool(mse < best_mse)                 # ref encode.py:108-117
        if improved:
            best, best_mse = params.clone(), mse
        mse_log[e - 1, 0], mse_log[e - 1, 1] = float(mse), float(improved)
    torch.cuda.synchronize()
    assert fit.evaluated == [1, 2, 3] and tuple(fit.losses.shape) == (EPOCHS, steps)
    assert torch.equal(fit.losses.view(torch.int32), losses.view(torch.int32))
    assert torch.equal(fit.mse_log.view(torch.int32), mse_log.view(torch.int32)) and bool(mse_log[0, 1] > 0)
    assert torch.equal(fit.best_params.view(torch.int32), best.view(torch.int32))
    # and it is another fit than the one that steps every pixel
    plain = _fit(dev, img, draws=dr)
    assert plain.n_valid is None and tuple(plain.losses.shape) == (EPOCHS, -(-H * W // BS)) and not torch.equal(plain.best_params, fit.best_params)


def test_groups_equal_the_single_fits(dev):
    dr = _draws()
    full, a, b = _tile("full"), _tile("collar"), _tile("collar2")
    full_d, a_d, b_d = (ops.to_device_u16(t, dev) for t in (full, a, b))
    single = {(name, k): _fit(dev, t, k, nodata=0, draws=dr) for name, t, k in (("full", full, 5), ("a", a, 4), ("a", a, 5), ("b", b, 5))}
    assert len({single[key].n_valid for key in (("full", 5), ("a", 5), ("b", 5))}) == 3 and single[("full", 5)].n_valid == 64 * 96
    # two K of one raster: one group, one ValidPixels, one permutation stream
    pair = codec.fit_group([a_d, a_d], [4, 5], D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), keep_losses=True, draws=[dr, dr], nodata=0)
    _same_fit(pair[0], single[("a", 4)])
    _same_fit(pair[1], single[("a", 5)])
    with pytest.raises(ValueError):      # one n_valid per group
        codec.fit_group([a_d, b_d], 5, D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), draws=[dr, dr], nodata=0)
    # fit_many: the jobs split where n_valid differs, the results come back in input order
    keys = [("full", 5), ("a", 4), ("a", 5), ("b", 5)]
    many = codec.fit_many([full_d, a_d, a_d, b_d], [k for _, k in keys], D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), in_flight=4, group=2,
                          draws=[dr] * 4, nodata=0)
    for got, key in zip(many, keys):
        assert got.n_valid == single[key].n_valid
        assert torch.equal(got.best_params.view(torch.int32), single[key].best_params.view(torch.int32))
        assert torch.equal(got.mse_log.view(torch.int32), single[key].mse_log.view(torch.int32)) and got.evaluated == [1, 2, 3]
    # one entry per image: the full tile without the argument is today's fit
    mixed = codec.fit_many([full_d, a_d], 5, D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), in_flight=2, group=1, draws=[dr] * 2, nodata=[None, 0])
    assert mixed[0].n_valid is None and mixed[1].n_valid == single[("a", 5)].n_valid
    assert torch.equal(mixed[0].best_params.view(torch.int32), single[("full", 5)].best_params.view(torch.int32))
    assert torch.equal(mixed[1].best_params.view(torch.int32), single[("a", 5)].best_params.view(torch.int32))


def test_a_tile_without_the_value_fits_as_it_does_today(dev):
    img = _tile("full")
    dr = _draws()
    for V in (0, 65535):
        assert not (img == V).any()
        with_v = _fit(dev, img, nodata=V, draws=dr)
        _same_fit(with_v, _fit(dev, img, draws=dr))
        assert with_v.n_valid == 64 * 96


def test_a_tile_of_nothing_but_the_value_runs_nothing(dev):
    dr = _draws()
    fit = _fit(dev, _tile("void"), nodata=0, draws=dr)
    torch.cuda.synchronize()
    assert fit.n_valid == 0 and fit.evaluated == [] and tuple(fit.losses.shape) == (EPOCHS, 0)
    assert torch.equal(fit.best_params.cpu().view(torch.int32), dr.params.view(torch.int32)) and not bool(fit.mse_log.any())
    both = codec.fit_group([ops.to_device_u16(_tile("void"), dev)] * 2, [4, 5], D, BC, NL, LR, BS, EPOCHS, cfg=FeatCfg(), keep_losses=True,
                           draws=[dr, dr], nodata=0)
    for f in both:
        assert f.n_valid == 0 and f.evaluated == [] and torch.equal(f.best_params.cpu().view(torch.int32), dr.params.view(torch.int32))


def test_command_lines_round_trip(dev, tmp_path):
    import decode
    import encode
    from lbdrn_hip import container, raster_io
    img = _tile("collar")
    src = str(tmp_path / "scene.npy")
    np.save(src, img)
    common = ["-i", src, "-e", str(EPOCHS), "-bs", str(BS), "-K", str(K)]
    n = int((~(img == 0).all(0)).sum())

    def run(name, extra):
        assert encode.main(common + ["-o", str(tmp_path / name)] + extra) == 0
        (sub,) = [d for d in (tmp_path / name).iterdir() if d.is_dir()]
        binp = str(sub / "scene.bin")
        assert decode.main(["-i", binp]) == 0
        return open(binp, "rb").read(), _records(str(sub / "encode.txt")), raster_io.read_raster(binp[:-4] + "_recon.tif").reshape(img.shape)

    with _settings(None, "LBB2", None):
        plain, recs_plain, _ = run("plain", ["--nodata", "0"])
        same, recs_same, _ = run("all", ["--nodata", "0", "--nodata-fit", "all"])
        valid, recs_valid, rec = run("valid", ["--nodata", "0", "--nodata-fit", "valid"])
        bounded, _, rec2 = run("bounded", ["--nodata", "0", "--nodata-fit", "valid", "--max-error", "2"])
    # `all` writes the file that leaving the option out writes, and its records
    strip = lambda rs, name: [r.replace(str(tmp_path / name), "X") for r in rs if not r.startswith(("Time elapsed", "Namespace")) and " fit " not in r]
    assert same == plain and strip(recs_same, "all") == strip(recs_plain, "plain")
    # `valid`: the one new record; the same format (read by the decoder above) and the same mask chunk; another fit (the weight
    # payload is entropy-coded: its size follows the weights)
    assert [r for r in recs_valid if r.startswith("Nodata fit")] == [f"Nodata fit: {n} of {64 * 96} pixels, {-(-n // BS)} steps per epoch"]
    assert not any(r.startswith("Nodata fit") for r in recs_plain + recs_same)
    assert valid != plain and container.unpack_nodata_trailer(valid) == container.unpack_nodata_trailer(plain)
    # decoded == V exactly where original == V, and nowhere else; with --max-error 2 the bound holds on every sample
    assert np.array_equal(rec == 0, img == 0) and np.array_equal(rec2 == 0, img == 0)
    assert int(np.abs(rec2.astype(np.int64) - img.astype(np.int64)).max()) <= 2
    assert np.array_equal(rec >> K, img >> K)
