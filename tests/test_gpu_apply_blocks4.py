"""The last layer of the tolerance-arithmetic evaluation pass on 4x4 MFMA blocks (k_apply_mfma, last_layer_4x4).

With C <= 8 the fast pass (LBDRN_EVAL_FAST, and its exact-operand variant LBDRN_EVAL_X16) sums the last layer as
bias + even units, odd units, then the two, on v_mfma_f32_4x4x1_16B_f32, its A operand read out of the fragments as they are
packed for the 32x32x2 step.  What can go wrong there is which fragment entry a lane reads (groups of four channels, the zero
rows past C), the join of the two lane halves, the bias seeded in one half only, and which channels each half finishes -- so:
every C whose last group is full or ragged, both widths of the hidden tile (bc = 32, 64), one and two hidden layers, both
window sizes, both activations, rasters with ragged edges in both directions and fewer rows than a tile, weights of mixed
magnitude with a last-layer bias large against the products.  The decode pass and the canonical evaluation keep their arithmetic (one k-ascending chain on 32x32x2, bit for bit the
oracle's: tests/test_gpu_parity.py and the decode tests), so nothing here restates them.  With more than 8 bands the fast
instances are never launched: the pass is the canonical one (or the streaming kernel's), and says so here."""
import numpy as np
import pytest
import torch

from lbdrn_hip import codec, ops
from lbdrn_hip.features import FeatCfg
from lbdrn_hip.synth import synthetic_tile

pytestmark = pytest.mark.gpu

RASTERS = [(17, 65), (5, 33), (64, 64)]   # ragged in both directions (2 x 2 tiles) / fewer rows than a tile, one ragged tile / 4 tiles


def _mixed_params(rng, F, bc, C, nl):
    """state_dict order; rows of every layer scaled by powers of two between 1/8 and 2, the last layer's between 1/16 and 4,
    and a last bias of up to +-4 beside products of a few hundredths (every other channel; the rest near zero)."""
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = 2.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0
        w = rng.uniform(-b, b, (bc, nin)) * np.exp2(rng.integers(-3, 2, (bc, 1)))
        parts += [w.ravel(), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0
    w = rng.uniform(-b, b, (C, bc)) * np.exp2(rng.integers(-4, 3, (C, 1)))
    bias = np.where(np.arange(C) % 2 == 0, rng.uniform(-4.0, 4.0, C), rng.uniform(-1e-3, 1e-3, C))
    parts += [w.ravel(), bias]
    return np.concatenate(parts).astype(np.float32)


_IMAGES = {}


def _image(C, H, W, dev):
    if (C, H, W) not in _IMAGES:
        img_d = ops.to_device_u16(synthetic_tile(100 + C, C, H, W), dev)
        _IMAGES[(C, H, W)] = (img_d,) + tuple(ops.split_bits(img_d, 5))
    return _IMAGES[(C, H, W)]


@pytest.mark.parametrize("bc", [32, 64])
@pytest.mark.parametrize("C", [2, 4, 6, 8])
def test_fast_pass_on_4x4_blocks_holds_the_canonical_sum(dev, C, bc):
    """(a) within 1e-6 relative of the canonical pass's float64 sum -- what the flag promises; (b) the same bits run to run
    and on the background launch's grid (half the workgroups, each walking two virtual ones: the nvirt contract).  Both
    for the fast pass and for its exact-operand variant (which is the fast pass where the shape does not qualify)."""
    cfg = FeatCfg()
    worst = 0.0
    for H, W in RASTERS:
        img_d, msb_d, mx = _image(C, H, W, dev)
        for D in (1, 2):
            geom = ops.FeatureGeometry(C, H, W, 5, D, mx, cfg, dev)
            F = cfg.feature_dim(C, D)
            for nl in (1, 2):
                for act in (ops.ACT_SINE, ops.ACT_RELU):
                    net = ops.make_net(F, bc, C, nl, act)
                    rng = np.random.default_rng(1000 * C + 100 * D + 10 * nl + act + bc)
                    p = torch.from_numpy(_mixed_params(rng, F, bc, C, nl)).to(dev)
                    canon = float(ops.eval_sse(geom, net, img_d, msb_d, p).item())
                    assert canon > 0
                    for x16 in (False, True):
                        fast = [float(ops.eval_sse(geom, net, img_d, msb_d, p, fast=True, x16=x16, background=b).item())
                                for b in (False, False, True)]
                        case = (C, bc, H, W, D, nl, act, x16)
                        assert fast[0] == fast[1] == fast[2], case
                        rel = abs(fast[0] - canon) / canon
                        worst = max(worst, rel)
                        assert rel <= 1e-6, (case, fast[0], canon)
    print(f"C={C} bc={bc}: worst |fast - canonical| / canonical = {worst:.3e}")


@pytest.mark.parametrize("shape", [(10, 64, 1, 2), (16, 64, 2, 2), (18, 32, 3, 1), (32, 32, 1, 1)])
def test_more_than_8_bands_never_reach_the_4x4_instances(dev, shape):
    """C > 8 (last_layer_4x4 finishes channels 0..7 only): a fast request is served by the canonical pass -- the same float64,
    run to run and on the background grid --, also in the exact-operand variant, on a ragged raster and both activations."""
    C, bc, D, nl = shape
    cfg = FeatCfg()
    H, W = 17, 65
    img_d, msb_d, mx = _image(C, H, W, dev)
    geom = ops.FeatureGeometry(C, H, W, 5, D, mx, cfg, dev)
    F = cfg.feature_dim(C, D)
    for act in (ops.ACT_SINE, ops.ACT_RELU):
        net = ops.make_net(F, bc, C, nl, act)
        p = torch.from_numpy(_mixed_params(np.random.default_rng(C + act), F, bc, C, nl)).to(dev)
        canon = float(ops.eval_sse(geom, net, img_d, msb_d, p).item())
        assert canon > 0
        for x16 in (False, True):
            for b in (False, True):
                assert float(ops.eval_sse(geom, net, img_d, msb_d, p, fast=True, x16=x16, background=b).item()) == canon, (shape, act, x16, b)


def test_fast_request_where_only_the_fast_plan_would_fit_in_lds(dev):
    """18 bands, D = 3, bc = 32, one layer, 7 positional features: the canonical plan of the LDS-resident kernel is a few
    hundred bytes over the 160 KB, the channel-pair plan of the fast pass would fit.  No fast plan is made for C > 8 and the
    library does not count the shape as one of the fused apply pass's (lbdrn_apply_workspace is the generic sizing), so the
    request is answered where the canonical one is, by the generic kernels: the same float64 -- never by a 4x4 instance, and
    not by an error."""
    C, bc, D, nl = 18, 32, 3, 1
    cfg = FeatCfg(True, True, 1.4, 3)
    H, W = 17, 65
    img_d, msb_d, mx = _image(C, H, W, dev)
    geom = ops.FeatureGeometry(C, H, W, 5, D, mx, cfg, dev)
    F = cfg.feature_dim(C, D)
    net = ops.make_net(F, bc, C, nl)
    p = torch.from_numpy(_mixed_params(np.random.default_rng(18), F, bc, C, nl)).to(dev)
    canon = float(ops.eval_sse(geom, net, img_d, msb_d, p).item())
    assert canon > 0
    fast = float(ops.eval_sse(geom, net, img_d, msb_d, p, fast=True).item())
    print(f"P={geom.c.P} F={F}: fast {fast!r} canonical {canon!r}")
    assert fast == canon


def test_small_fit_ranks_its_epochs_as_the_canonical_evaluation_does(dev, monkeypatch):
    """(c) a whole small fit (4 x 64 x 64, 3 epochs): the float32 MSEs it logs and the epoch it keeps are those of the same
    fit with its evaluation passes in the canonical arithmetic (LBDRN_EVAL_CANONICAL)."""
    img_d = ops.to_device_u16(synthetic_tile(104, 4, 64, 64), dev)
    fits = []
    for canonical in ("0", "1"):
        monkeypatch.setenv("LBDRN_EVAL_CANONICAL", canonical)
        torch.manual_seed(19920517)
        fits.append(codec.fit_device(img_d, 5, 2, 64, 2, 1e-3, 256, 3))
    a, b = fits
    print("mse_log fast     :", a.mse_log.cpu().numpy().tolist())
    print("mse_log canonical:", b.mse_log.cpu().numpy().tolist())
    assert torch.equal(a.mse_log[:, 1], b.mse_log[:, 1])
    assert torch.equal(a.best_params.view(torch.int32), b.best_params.view(torch.int32))
    assert torch.equal(a.mse_log[:, 0], b.mse_log[:, 0])
