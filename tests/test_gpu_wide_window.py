"""The wide fused training step: bc = 64, two hidden layers, 256 < Fe <= 384 features multiplied -- D = 3 windows on 6, 7
or 8 bands with relative colours (the reference's run.sh D3 sweep on its 8-band images: F = 392, Fe = 384) -- on
k_train_split<96, 24>, W_0 passing through a 12-group ring in LDS (csrc/train_split.inc)."""
import os

import numpy as np
import pytest
import torch

import oracle as O
from lbdrn_hip import codec, ops
from lbdrn_hip.features import FeatCfg
from train_step_f64 import f64_steps

pytestmark = pytest.mark.gpu
GEN, MFMA, AUTO = ops._lib.PATH_GENERIC, ops._lib.PATH_MFMA, ops.PATH_AUTO
RTOL_TRAIN = 1e-5


def _params(rng, F, bc, C, nl, gain):
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = (1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


def _shape(img, K, D, cfg, dev):
    C, H, W = img.shape
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(cfg.feature_dim(C, D), 64, C, 2, cfg.act)
    return img_d, msb_d, geom, net


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _f64_steps(x, t, params0, batches, F, bc, C, lrs, act):
    """The teacher-forced updates in float64 numpy (tests/train_step_f64.py)."""
    return f64_steps(x, t, params0, batches, F, bc, C, lrs, act=act, nl=2)


def _teacher_forced(dev, img, cfg, params0, batches, lrs, rows, path, alone, losses_ref=None):
    """lbdrn_train_epoch fed a fixture's minibatches, the ones of one learning rate per call; every loss checked."""
    img_d, msb_d, geom, net = _shape(img, 5, 3, cfg, dev)
    assert ops.train_step_features(geom, net) == 384
    p = torch.from_numpy(params0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = ops.TrainWorkspace(geom, net, rows, dev).prepare(img_d, msb_d, path)
    s = 0
    while s < len(batches):
        e = s
        while e < len(batches) and lrs[e] == lrs[s]:
            e += 1
        perm = torch.from_numpy(np.concatenate(batches[s:e])).to(dev)
        losses = torch.zeros(e - s, dtype=torch.float32, device=dev)
        ops.train_epoch(geom, net, img_d, msb_d, perm, rows, p, m, v, s, float(lrs[s]), losses, path, ws, alone=alone)
        if losses_ref is not None:
            for k in range(s, e):
                assert abs(float(losses[k - s].item()) - float(losses_ref[k])) <= RTOL_TRAIN * float(losses_ref[k]), k
        s = e
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("alone", (False, True))
@pytest.mark.parametrize("tag,rows", (("small", 96), ("ragged", 200), ("relu", 96)))
def test_d3_bands8_fused_step_matches_reference_fixture(golden, dev, tag, rows, alone):
    """tests/golden/make_golden_d3.py: the reference's LBDRNModel(392, 64, 8, 2), six teacher-forced Adam steps.  Every loss
    within 1e-5, the parameters within 2e-5 of the reference run, and no farther from the float64 evaluation of the same steps
    than the generic step (or the reference's own float32 run) is."""
    G = golden["d3_bands8"]
    img = G[("ragged" if tag == "ragged" else "small") + "/img"]
    act = "relu" if tag == "relu" else "sine"
    cfg = FeatCfg(activation=act)
    batches, lrs = list(G[tag + "/batches"]), [float(x) for x in G[tag + "/lrs"]]
    assert len(batches[0]) == rows
    p, m, v = _teacher_forced(dev, img, cfg, G["params0"], batches, lrs, rows, MFMA, alone, G[tag + "/losses"])
    pr = G[tag + "/step5/params"]
    assert np.linalg.norm(p - pr) <= 2e-5 * np.linalg.norm(pr)
    msb, lab, mx = O.split_bits(img, 5)
    feats = O.features(msb, 3, O.FeatCfg(), mx)
    assert feats.shape[1] == 392
    p64, _, _ = _f64_steps(feats, lab, G["params0"], batches, 392, 64, 8, lrs, act)
    pg, _, _ = _teacher_forced(dev, img, cfg, G["params0"], batches, lrs, rows, GEN, alone)
    # (the fused step takes sin / cos / sigmoid from the hardware behind a compensated reduction, 4.5e-7 absolute, where the
    #  generic step uses the canonical polynomials: csrc/train_mfma.hip, train_sincos.  Measured on "small": 2.3e-6 from the
    #  float64 run against 0.8e-6 for the generic step and 0.6e-6 for the reference's float32 run, in a vector of norm 0.54)
    err, err_gen, err_ref = (np.linalg.norm(a - p64) for a in (p, pg, pr))
    assert err <= max(2 * err_gen, 2 * err_ref) + 5e-6 * np.linalg.norm(p64), (err, err_gen, err_ref)
    if tag == "small":   # the first step's gradient (exp_avg = 0.1 g after one step) and the moments at the end
        assert np.array_equal(lab, G["small/labels"])
        _, m1, _ = _teacher_forced(dev, img, cfg, G["params0"], batches[:1], lrs[:1], rows, MFMA, alone)
        g = G["small/step0/grads"]
        assert np.abs(10.0 * m1 - g).max() <= 2e-5 * np.abs(g).max()
        for name, hip in (("exp_avg", m), ("exp_avg_sq", v)):
            ref = G["small/" + name]
            assert np.abs(hip - ref).max() <= 1e-4 * np.abs(ref).max(), name


def _epoch(dev, geom, net, img_d, msb_d, perm_np, bs, p0, path, alone=False, ws=None, epochs=1):
    perm = torch.from_numpy(perm_np).to(dev)
    steps = (len(perm_np) + bs - 1) // bs
    p = torch.from_numpy(p0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    for e in range(epochs):
        ops.train_epoch(geom, net, img_d, msb_d, perm, bs, p, m, v, e * steps, 1e-3, losses, path, ws, alone=alone)
    return [t.cpu().numpy() for t in (p, losses, m, v)]


def test_wide_window_fuzz(dev):
    """C = 6, 7, 8 at D = 3 (Fe = 288, 336, 384), either activation, random sizes and K, minibatches of 1, 31, 33, 257 and
    H W +- k rows: MFMA against generic within test_gpu_fuzz's tolerances; the fused step reproducible bit for bit, alone
    equal to not alone, a group of two equal to two single calls."""
    rng = np.random.default_rng(20261016)
    sizes = [1, 31, 33, 257, -3, 10 ** 4, 1, 257, 33, -1, 31, 3]   # (< 0: H W minus that; 10^4: one minibatch, H W plus some)
    for it, bsel in enumerate(sizes):
        C = (6, 7, 8)[it % 3]
        act = "relu" if it % 4 == 3 else "sine"
        cfg = FeatCfg(activation=act)
        H, W, K = int(rng.integers(7, 30)), int(rng.integers(7, 40)), int(rng.integers(1, 8))
        if bsel == 1:
            H, W = min(H, 12), min(W, 15)   # (a one-row minibatch is one launch per row)
        N = H * W
        bs = bsel if bsel > 0 else N + bsel
        img = rng.integers(0, 1 << int(rng.integers(K + 2, 15)), (C, H, W)).astype(np.uint16)
        img[0, 0, 0] |= np.uint16(1 << K)   # (an MSB plane that is not all zero)
        imgs = [img, np.ascontiguousarray(np.roll(img, (3, 5), axis=(1, 2)))]   # (the group's second fit: same shape and maximum)
        shapes = [_shape(im, K, 3, cfg, dev) for im in imgs]
        img_d, msb_d, geom, net = shapes[0]
        F = cfg.feature_dim(C, 3)
        assert ops.train_step_features(geom, net) == C * 48
        p0 = _params(rng, F, 64, C, 2, 10.0 if cfg.act else 1.0)
        order = rng.permutation(N).astype(np.int64)
        tag = (it, C, H, W, K, bs, act)
        # one (usually ragged) step, then a few ending ragged: the tolerances of test_train_fuzz_mfma_matches_generic
        one = order[:int(rng.integers(1, min(bs, N) + 1))]
        (pa, la, ma, va), (pb, lb, mb, vb) = (_epoch(dev, geom, net, img_d, msb_d, one, bs, p0, path) for path in (MFMA, GEN))
        np.testing.assert_allclose(la, lb, rtol=2e-5, err_msg=str(tag))
        assert np.abs(ma - mb).max() <= 2e-5 * np.abs(mb).max(), tag
        assert np.abs(va - vb).max() <= 5e-5 * np.abs(vb).max(), tag
        few = order[:min(N, 5 * bs + int(rng.integers(1, bs + 1)))]
        (pa, la, ma, va), (pb, lb, mb, vb) = (_epoch(dev, geom, net, img_d, msb_d, few, bs, p0, path) for path in (MFMA, GEN))
        nsteps = len(la)
        np.testing.assert_allclose(la, lb, rtol=5e-5, err_msg=str(tag))
        assert np.linalg.norm(pa - pb) <= 0.01 * 1e-3 * nsteps * np.sqrt(len(pa)), tag
        assert np.isfinite(pa).all(), tag
        # bits: twice the same, alone = not alone (two epochs each)
        ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img_d, msb_d, MFMA)
        runs = [_epoch(dev, geom, net, img_d, msb_d, order, bs, p0, MFMA, alone, ws, epochs=2) for alone in (False, False, True)]
        assert _bits_equal(runs[0], runs[1]) and _bits_equal(runs[0], runs[2]), tag
        # a group of two fits = two single calls
        perms = [torch.from_numpy(order).to(dev), torch.from_numpy(rng.permutation(N).astype(np.int64)).to(dev)]
        steps = (N + bs - 1) // bs
        singles = [runs[0]] + [_epoch(dev, shapes[1][2], net, shapes[1][0], shapes[1][1], perms[1].cpu().numpy(), bs, p0, MFMA, epochs=2)]
        ps = [torch.from_numpy(p0.copy()).to(dev) for _ in range(2)]
        ms, vs = [torch.zeros_like(ps[0]) for _ in range(2)], [torch.zeros_like(ps[0]) for _ in range(2)]
        ls = [torch.zeros(steps, dtype=torch.float32, device=dev) for _ in range(2)]
        wss = [ops.TrainWorkspace(g, net, bs, dev).prepare(i, m_, MFMA) for (i, m_, g, _) in shapes]
        for e in range(2):
            ops.train_epoch_group([s[2] for s in shapes], net, [s[0] for s in shapes], [s[1] for s in shapes], perms, bs,
                                  ps, ms, vs, e * steps, 1e-3, ls, MFMA, wss)
        for k in range(2):
            got = [t.cpu().numpy() for t in (ps[k], ls[k], ms[k], vs[k])]
            assert _bits_equal(got, singles[k]), (tag, k)


def test_wide_window_slabs_past_2gib(dev):
    """A minibatch whose gradient slabs pass 2 GiB (k_reduce_adam addresses them with 32-bit offsets): 117 KB of slab per 32
    rows at this shape, so 573,600 rows and more.  PATH_MFMA refuses it, PATH_AUTO steps on the generic kernels."""
    rng = np.random.default_rng(5)
    C, H, W, K = 8, 760, 760, 5
    img = rng.integers(0, 4096, (C, H, W)).astype(np.uint16)
    cfg = FeatCfg()
    img_d, msb_d, geom, net = _shape(img, K, 3, cfg, dev)
    bs = H * W
    p0 = _params(rng, cfg.feature_dim(C, 3), 64, C, 2, 1.0)
    order = rng.permutation(H * W).astype(np.int64)
    with pytest.raises(ops._lib.LbdrnError):
        _epoch(dev, geom, net, img_d, msb_d, order, bs, p0, MFMA)
    a = _epoch(dev, geom, net, img_d, msb_d, order, bs, p0, AUTO)
    b = _epoch(dev, geom, net, img_d, msb_d, order, bs, p0, GEN)
    assert _bits_equal(a, b)


def test_wide_window_full_tile_in_flight_equals_alone(dev):
    """One 8 x 2048^2 tile at D = 3 (6.7 GB of rows a fit), two fits of two epochs: fit_many with two in flight (a group
    of two on one launch per minibatch) ends on the same bits as the same fits run one at a time; the losses are finite
    and fall."""
    from lbdrn_hip.synth import synthetic_tile
    imgs = [ops.to_device_u16(synthetic_tile(s, 8, 2048, 2048), dev) for s in (11, 12)]
    kw = dict(K=5, D=3, base_channel=64, num_layers=2, lr=1e-3, batch_size=8192, epochs=2)
    both = codec.fit_many(imgs, in_flight=2, group=2, **kw)
    one = [codec.fit_many([im], in_flight=1, **kw)[0] for im in imgs]
    for a, b in zip(both, one):
        assert torch.equal(a.best_params.view(torch.int32), b.best_params.view(torch.int32))
        assert torch.equal(a.mse_log, b.mse_log)
        mse = a.mse_log[:, 0].cpu().numpy()
        assert np.isfinite(mse).all() and mse[-1] < mse[0], mse


def test_wide_window_lone_fit_schedule_changes_no_bit(dev, monkeypatch):
    """A lone fit of the wide shape with its evaluation passes in the background of the next epoch's training
    (LBDRN_OVERLAP_EVAL=1) and in the chain (=0): the same best weights, the same epoch log."""
    from lbdrn_hip.synth import synthetic_tile
    img = ops.to_device_u16(synthetic_tile(3, 8, 256, 320), dev)
    fits = []
    for flag in ("0", "1"):
        monkeypatch.setenv("LBDRN_OVERLAP_EVAL", flag)
        torch.manual_seed(19920517)
        fits.append(codec.fit_device(img, 5, 3, 64, 2, 1e-3, 4096, 4))
    a, b = fits
    assert torch.equal(a.best_params.view(torch.int32), b.best_params.view(torch.int32))
    assert torch.equal(a.mse_log, b.mse_log)


def test_wide_window_encode_decode_round_trip(dev, tmp_path, monkeypatch):
    """encode.py / decode.py -D 3 on a synthetic 8-band image: the fused wide step trains it, the written raster keeps the
    high bits and equals the oracle's decode of the payload in the file."""
    import decode
    import encode
    from lbdrn_hip import container, raster_io
    from lbdrn_hip.synth import synthetic_tile
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    img = synthetic_tile(7, 8, 64, 96)
    src = str(tmp_path / "img.npy")
    np.save(src, img)
    out = str(tmp_path / "o")
    assert encode.main(["-i", src, "-o", out, "-K", "5", "-D", "3", "-bs", "1024", "-e", "3"]) == 0
    sub = os.listdir(out)[0]
    binp = os.path.join(out, sub, "img.bin")
    hdr = container.unpack_header(open(binp, "rb").read())
    assert hdr[7] == 3
    assert decode.main(["-i", binp]) == 0
    rec = raster_io.read_raster(os.path.join(out, sub, "img_recon.tif")).reshape(img.shape)
    assert np.array_equal(rec >> 5, img >> 5)
    assert not np.array_equal(rec, (img >> 5) << 5)   # (the residual network wrote low bits)


def test_x16_hint_at_d3_eight_bands_is_the_fast_pass(dev):
    """LBDRN_EVAL_X16 is a hint: at C = 8, D = 3, bc = 64 the x16 weight pack does not fit in LDS beside the window tile,
    so the pass is the fast one, bit for bit (it used to fail with LBDRN_E_UNSUPPORTED)."""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 4000, (8, 40, 70)).astype(np.uint16)
    cfg = FeatCfg()
    img_d, msb_d, geom, net = _shape(img, 5, 3, cfg, dev)
    p = torch.from_numpy(_params(rng, cfg.feature_dim(8, 3), 64, 8, 2, 3.0)).to(dev)
    fast = float(ops.eval_sse(geom, net, img_d, msb_d, p, fast=True).item())
    for b in (False, True):
        x16 = float(ops.eval_sse(geom, net, img_d, msb_d, p, fast=True, x16=True, background=b).item())
        assert x16 == fast, (b, x16, fast)
