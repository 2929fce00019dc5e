"""Parity of the HIP path (through the C ABI) against the oracle: bit-exact for integer / byte work
and for the canonical-arithmetic forward, 1e-5 relative for the training step."""
import numpy as np
import pytest
import torch

import oracle as O
from lbdrn_hip import ops
from lbdrn_hip.features import FeatCfg
from train_step_f64 import f64_steps

pytestmark = pytest.mark.gpu

RTOL_TRAIN = 1e-5  # north_star: encode-time float loss within 1e-5 relative


def _cfg(flags):
    return FeatCfg(use_coordinates=bool(flags[0]), embedding=bool(flags[1]),
                   use_colors=bool(flags[2]), relative=bool(flags[3]))


def _ocfg(c):
    return O.FeatCfg(c.use_coordinates, c.embedding, c.sigma, c.n_freq, c.use_colors, c.relative)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rand_params(rng, F, bc, C, nl, gain=1.0):
    """SIREN-like magnitudes so that sin(30 z) wraps a few times."""
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = (1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


def _image(rng, C, H, W, hi=10000):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.empty((C, H, W), np.uint16)
    for c in range(C):
        a = np.sin(yy / (3.0 + c) + xx / (5.0 + 2 * c) + c) * 0.4 + 0.5
        img[c] = np.clip(a * hi + rng.normal(0, hi * 0.01, (H, W)), 0, hi).astype(np.uint16)
    return img


# ---------------------------------------------------------------- a1-a3

def test_split_labels_features_match_oracle_on_golden_cases(golden, dev):
    G = golden["features"]
    for name in sorted({k.split("/")[0] for k in G.files}):
        img, K, D = G[name + "/img"], int(G[name + "/K"]), int(G[name + "/D"])
        cfg = _cfg(G[name + "/flags"])
        img_d = ops.to_device_u16(img, dev)
        msb_d, mx = ops.split_bits(img_d, K)
        msb_o, lab_o, mx_o = O.split_bits(img, K)
        assert mx == mx_o
        assert np.array_equal(ops.from_device_u16(msb_d), msb_o)
        lab = ops.labels(img_d, K).cpu().numpy()
        assert np.array_equal(_bits(lab), _bits(G[name + "/labels"])), name
        C, H, W = img.shape
        geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
        f = ops.features(geom, msb_d).cpu().numpy()
        assert f.shape == G[name + "/features"].shape
        assert np.array_equal(_bits(f), _bits(G[name + "/features"])), name  # reference bits
        idx = torch.tensor([H * W - 1, 0, W, 3, H * W // 2], dtype=torch.int64, device=dev)
        fi = ops.features(geom, msb_d, idx).cpu().numpy()
        assert np.array_equal(_bits(fi), _bits(G[name + "/features"][idx.cpu().numpy()]))
        li = ops.labels(img_d, K, idx).cpu().numpy()
        assert np.array_equal(_bits(li), _bits(G[name + "/labels"][idx.cpu().numpy()]))


# ---------------------------------------------------------------- a5

@pytest.mark.parametrize("F,bc,C,nl,B", [(200, 64, 8, 2, 777), (18, 16, 3, 3, 65), (50, 32, 4, 1, 1),
                                         (250, 256, 8, 2, 130), (7, 8, 1, 2, 64)])
def test_forward_bit_exact_vs_oracle(dev, F, bc, C, nl, B):
    rng = np.random.default_rng(F * 7 + bc)
    params = _rand_params(rng, F, bc, C, nl, gain=3.0)
    x = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    y = ops.forward(ops.make_net(F, bc, C, nl), torch.from_numpy(params).to(dev),
                    torch.from_numpy(x).to(dev)).cpu().numpy()
    yo = O.forward(params, F, bc, C, nl, x)
    assert np.array_equal(_bits(y), _bits(yo))


def test_forward_matches_reference_fixture(golden, dev):
    G = golden["forward"]
    for case in ("init", "wide", "embed"):
        x, p, y_ref = G[case + "/x"], G[case + "/params"], G[case + "/y"]
        net = ops.make_net(x.shape[1], 64, 8, 2)
        y = ops.forward(net, torch.from_numpy(p).to(dev), torch.from_numpy(x).to(dev)).cpu().numpy()
        np.testing.assert_allclose(y, y_ref, rtol=1e-5, atol=1e-6)


def test_model_forward_drop_in(golden, dev):
    from LBDRNmodel import LBDRNModel
    G = golden["forward"]
    torch.manual_seed(19920517)
    m = LBDRNModel(dim_in=200, dim_hidden=64, dim_out=8, num_layers=2)
    assert np.array_equal(m.flat_parameters().numpy(), G["init/params"])
    m = m.to(dev)
    y = m(torch.from_numpy(G["init/x"]).to(dev)).cpu().numpy()
    np.testing.assert_allclose(y, G["init/y"], rtol=1e-5, atol=1e-6)
    with pytest.raises(Exception):
        m(torch.from_numpy(G["init/x"]))  # CPU tensor: no CPU path


# ---------------------------------------------------------------- a2+a5+a11, a9

APPLY_CASES = [
    # C, H, W, K, D, bc, nl, flags(coords, embed, colors, relative)
    (8, 37, 150, 5, 2, 64, 2, (0, 0, 1, 1)),
    (8, 16, 64, 5, 2, 64, 2, (0, 0, 1, 1)),
    (3, 21, 33, 3, 1, 32, 1, (0, 0, 1, 1)),
    (4, 19, 70, 6, 0, 64, 3, (0, 0, 1, 1)),
    (1, 40, 41, 1, 3, 64, 2, (0, 0, 1, 1)),
    (5, 9, 129, 5, 2, 128, 2, (0, 0, 1, 0)),
    (8, 20, 66, 5, 2, 64, 2, (1, 1, 1, 1)),
    (8, 18, 35, 5, 2, 64, 2, (1, 0, 1, 1)),
    (4, 12, 65, 4, 2, 64, 2, (1, 1, 0, 1)),
    (2, 3, 4, 6, 2, 64, 2, (0, 0, 1, 1)),
    (8, 24, 20, 5, 2, 256, 2, (0, 0, 1, 1)),   # bc=256 (BASELINE configs[2]): the streaming kernel k_apply_wide
    (8, 21, 70, 5, 2, 256, 2, (1, 1, 1, 1)),   # bc=256 with the positional embedding (F=250: a group mixes both kinds)
    (3, 19, 131, 4, 1, 256, 1, (1, 0, 1, 0)),  # bc=256, one hidden layer, coords without embedding, ragged tiles
    (16, 9, 40, 6, 0, 256, 2, (0, 0, 1, 1)),   # bc=256, D=0, all 16 output slots
    (8, 24, 20, 5, 2, 256, 3, (0, 0, 1, 1)),   # bc=256 nl=3: generic path only
]


@pytest.mark.parametrize("case", APPLY_CASES)
def test_decode_and_eval_bit_exact_vs_oracle(dev, case):
    C, H, W, K, D, bc, nl, flags = case
    rng = np.random.default_rng(sum(case[:7]))
    cfg = _cfg(flags)
    img = _image(rng, C, H, W)
    msb_o, lab_o, mx = O.split_bits(img, K)
    F = cfg.feature_dim(C, D)
    params = _rand_params(rng, F, bc, C, nl, gain=2.0)
    out_o, y_o = O.decode(msb_o, K, D, _ocfg(cfg), params, bc, nl, mx, want_y=True)
    sse_o = O.eval_sse(msb_o, lab_o, D, _ocfg(cfg), params, bc, nl, mx)
    img_d, msb_d = ops.to_device_u16(img, dev), ops.to_device_u16(msb_o, dev)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(F, bc, C, nl)
    p_d = torch.from_numpy(params).to(dev)
    fused = bc <= 128 or nl <= 2
    paths = [ops._lib.PATH_GENERIC] + ([ops._lib.PATH_MFMA] if fused else [])
    for path in paths:
        out, y = ops.decode_fused(geom, net, msb_d, p_d, want_y=True, path=path)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(y_o)), (case, path)
        assert np.array_equal(ops.from_device_u16(out), out_o), (case, path)
        sse = float(ops.eval_sse(geom, net, img_d, msb_d, p_d, path=path).item())
        assert abs(sse - sse_o) <= 1e-11 * max(1.0, abs(sse_o)), (case, path, sse, sse_o)
    if not fused:
        with pytest.raises(ops._lib.LbdrnError):
            ops.decode_fused(geom, net, msb_d, p_d, path=ops._lib.PATH_MFMA)


def test_decode_matches_reference_fixture(golden, dev):
    """decode.py:122-134 replayed with the reference's model: identical raster on the fixture."""
    G = golden["decode"]
    img, K, D = G["img"], int(G["K"]), int(G["D"])
    msb, _, mx = O.split_bits(img, K)
    C, H, W = img.shape
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, FeatCfg(), dev)
    net = ops.make_net(200, 64, 8, 2)
    for path in (ops._lib.PATH_GENERIC, ops._lib.PATH_MFMA):
        out, y = ops.decode_fused(geom, net, ops.to_device_u16(msb, dev),
                                  torch.from_numpy(G["params"]).to(dev), want_y=True, path=path)
        np.testing.assert_allclose(y.cpu().numpy(), G["y"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(ops.from_device_u16(out), G["image"])


@pytest.mark.parametrize("tag", ("bc64", "bc256", "embed"))
def test_decode_big_rasters_hip_oracle_reference(golden, dev, tag):
    """524,288 sub-pixels per case, weights from 56 real torch Adam steps on the reference model, raster from the
    replay of decode.py:122-134 (tests/golden/make_golden_rasters.py), BASELINE configs[1]/[2]/[4] shapes:
    HIP == oracle bit for bit on every path, and HIP may differ from the REFERENCE raster only at sub-pixels
    within 1e-5 (in y) of a rounding boundary -- the number that do is bounded (measured 0, 0 and 1 of 524,288)."""
    G = golden["rasters_" + tag]
    img, K, D, bc, nl = G["img"], int(G["K"]), int(G["D"]), int(G["bc"]), int(G["nl"])
    cfg = _cfg(G["flags"])
    msb, _, mx = O.split_bits(img, K)
    C, H, W = img.shape
    out_o = O.decode(msb, K, D, _ocfg(cfg), G["params"], bc, nl, mx)
    ref = ((img >> K) << K) + G["residual"]
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(cfg.feature_dim(C, D), bc, C, nl)
    p_d, msb_d = torch.from_numpy(G["params"]).to(dev), ops.to_device_u16(msb, dev)
    for path in (ops._lib.PATH_GENERIC, ops._lib.PATH_AUTO, ops._lib.PATH_MFMA):
        out = ops.from_device_u16(ops.decode_fused(geom, net, msb_d, p_d, path=path))
        assert np.array_equal(out, out_o), (tag, path)
        bad = np.flatnonzero((out != ref).transpose(1, 2, 0).reshape(-1))
        assert np.isin(bad, G["near_idx"]).all(), (tag, path)
        # measured: 0 flips on bc64 and bc256, 1 on embed (an exact tie in the reference's y*31); at most 2 per
        # case, each within 4e-5 of the boundary in y*31 (1.3e-6 in y)
        assert bad.size <= 2, f"{tag}: {bad.size} boundary flips vs the reference of {out.size} sub-pixels"
        assert all(float(G["near_dist"][np.searchsorted(G["near_idx"], b)]) < 4e-5 for b in bad)


@pytest.mark.parametrize("tag", ("bc64", "bc256", "embed", "scaled"))
def test_decode_learnable_rasters_hip_oracle_reference(golden, dev, tag):
    """The rasters of tests/golden/make_golden_round3.py -- fits that DO predict the low bits (residuals over 0..31,
    PSNR 9-11 dB above "predict mid-range") and, for "scaled", sin arguments up to 361: HIP == oracle bit for bit on
    every path; HIP differs from the reference raster only at listed near-boundary sub-pixels."""
    G = golden["rasters_learn_" + tag]
    img, K, D, bc, nl = G["img"], int(G["K"]), int(G["D"]), int(G["bc"]), int(G["nl"])
    cfg = _cfg(G["flags"])
    msb, _, mx = O.split_bits(img, K)
    C, H, W = img.shape
    out_o = O.decode(msb, K, D, _ocfg(cfg), G["params"], bc, nl, mx)
    ref = ((img >> K) << K) + G["residual"]
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(cfg.feature_dim(C, D), bc, C, nl)
    p_d, msb_d = torch.from_numpy(G["params"]).to(dev), ops.to_device_u16(msb, dev)
    for path in (ops._lib.PATH_GENERIC, ops._lib.PATH_AUTO, ops._lib.PATH_MFMA):
        out = ops.from_device_u16(ops.decode_fused(geom, net, msb_d, p_d, path=path))
        assert np.array_equal(out, out_o), (tag, path)
        bad = np.flatnonzero((out != ref).transpose(1, 2, 0).reshape(-1))
        assert np.isin(bad, G["near_idx"]).all(), (tag, path)
        assert bad.size <= (16 if tag == "scaled" else 2)


# ---------------------------------------------------------------- a7, a8

def _fused_steps_vs_fixture(dev, img, cfg, bc, params0, batches, lrs, losses_ref, bs, alone=False):
    """lbdrn_train_epoch(PATH_MFMA) fed a fixture's minibatches, `per` of them per call with one learning rate (the
    fixture's "epochs"); returns (params, exp_avg, exp_avg_sq) after the last one, having checked every loss.
    alone: with the LBDRN_TRAIN_ALONE hint -- k_train_split steps where the shape has it (the kernel every `encode.py -sr 1`
    call trains on), so that it eats the reference's fixtures itself and not by transitivity."""
    C, H, W = img.shape
    K, D = 5, 2
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(cfg.feature_dim(C, D), bc, C, 2)
    p = torch.from_numpy(params0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img_d, msb_d, ops._lib.PATH_MFMA)
    s = 0
    while s < len(batches):
        e = s
        while e < len(batches) and lrs[e] == lrs[s]:
            e += 1
        perm = torch.from_numpy(np.concatenate(batches[s:e])).to(dev)
        losses = torch.zeros(e - s, dtype=torch.float32, device=dev)
        ops.train_epoch(geom, net, img_d, msb_d, perm, bs, p, m, v, s, float(lrs[s]), losses, ops._lib.PATH_MFMA, ws, alone=alone)
        for k in range(s, e):
            assert abs(float(losses[k - s].item()) - float(losses_ref[k])) <= RTOL_TRAIN * float(losses_ref[k]), k
        s = e
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def _f64_steps(x, t, params0, batches, F, bc, C, lrs):
    """The same teacher-forced updates in float64 numpy (tests/train_step_f64.py): what exact arithmetic gives, to tell a
    kernel's rounding from the reference run's own."""
    return f64_steps(x, t, params0, batches, F, bc, C, lrs, act="sine", nl=2)


def _as_close_to_float64_as_the_reference(name, hip, ref32, ref64):
    """max |hip - float64| against max |reference float32 run - float64|, both relative to the largest entry: the
    kernel may be as far from exact arithmetic as the reference's own run is (x2), or within 1e-5 outright."""
    scale = np.abs(ref64).max()
    err_ref, err_hip = np.abs(ref32 - ref64).max() / scale, np.abs(hip - ref64).max() / scale
    assert err_hip <= max(1e-5, 2 * err_ref), (name, err_hip, err_ref)
    return err_ref


def test_wide_train_kernel_matches_reference_fixture(golden, dev):
    """BASELINE.json configs[2]'s training kernel (k_train_wide, bc = 256) eats the reference's train256 fixture: image
    A_K5_D2's rows, the fixture's three 128-row minibatches through lbdrn_train_epoch(PATH_MFMA).  Loss within 1e-5
    at every step and final parameters within 2e-5 of the reference run.  The Adam moments are held to what float32
    can give at this width: the reference's own float32 run sits 5.3e-5 (exp_avg) / 6.8e-5 (exp_avg_sq) of the largest
    moment away from the same three steps evaluated in float64 (dots of 256 terms, sin(30 z) in between), so the
    kernel is measured against the float64 values and must be as close to them as the reference run is (x2)."""
    G, T2, Ft = golden["wide_net"], golden["train2"], golden["features"]
    batches = list(G["train256/batches"])
    p, m, v = _fused_steps_vs_fixture(dev, Ft["A_K5_D2/img"], FeatCfg(), 256, G["train256/params0"], batches,
                                      [1e-3] * 3, [G[f"train256/step{s}/loss"] for s in range(3)], 128)
    pr = G["train256/params_final"]
    assert np.linalg.norm(p - pr) <= 2e-5 * np.linalg.norm(pr)
    p64, m64, v64 = _f64_steps(Ft["A_K5_D2/features"], Ft["A_K5_D2/labels"], G["train256/params0"], batches, 200, 256, 8, [1e-3] * 3)
    for name, hip, ref32, ref64 in (("exp_avg", m, T2["wide256/exp_avg"], m64), ("exp_avg_sq", v, T2["wide256/exp_avg_sq"], v64)):
        err_ref = _as_close_to_float64_as_the_reference(name, hip, ref32, ref64)
        assert 2e-5 < err_ref < 1e-4, (name, err_ref)          # the fixture's own float32 rounding, as measured
    assert np.linalg.norm(p - p64) <= 2 * np.linalg.norm(pr - p64) + 1e-6 * np.linalg.norm(p64)


@pytest.mark.parametrize("alone", (False, True))
def test_embedding_train_kernel_matches_reference_fixture(golden, dev, alone):
    """(alone: k_train_split<64, 16> instead of k_train_stream<64, 2, 3, 16>.)  BASELINE.json configs[4]'s training kernel (the streamed step at LQ = 64, F = 250: coordinates + Fourier
    embedding ahead of the colours) eats a reference fixture of its own: six teacher-forced 96-row updates on an
    8 x 24 x 20 image, StepLR chain included -- loss 1e-5 per step, parameters 1e-5, and Adam moments as close to
    the float64 evaluation of the same six steps as the reference's float32 run is (x2; measured: the reference
    2e-5 of the largest moment, a few entries of 20,744)."""
    T = golden["train2"]
    cfg = _cfg(T["embed/flags"])
    lrs = [float(T[f"embed/step{s}/lr"]) for s in range(6)]
    batches = list(T["embed/batches"])
    p, m, v = _fused_steps_vs_fixture(dev, T["embed/img"], cfg, 64, T["embed/params0"], batches, lrs,
                                      [T[f"embed/step{s}/loss"] for s in range(6)], 96, alone=alone)
    pr = T["embed/step5/params"]
    assert np.linalg.norm(p - pr) <= 1e-5 * np.linalg.norm(pr)
    msb, lab, mx = O.split_bits(T["embed/img"], 5)
    feats = O.features(msb, 2, _ocfg(cfg), mx)          # (bit-identical to the reference's process(): test_oracle_golden)
    p64, m64, v64 = _f64_steps(feats, lab, T["embed/params0"], batches, 250, 64, 8, lrs)
    _as_close_to_float64_as_the_reference("exp_avg", m, T["embed/exp_avg"], m64)
    _as_close_to_float64_as_the_reference("exp_avg_sq", v, T["embed/exp_avg_sq"], v64)


@pytest.mark.parametrize("alone", (False, True))
def test_fused_train_kernel_matches_reference_fixture(golden, dev, alone):
    """(alone: k_train_split<48, 12> -- what a lone `encode.py -sr 1` fit steps on -- instead of k_train_stream.)
    The fused training kernels themselves (lbdrn_train_epoch, PATH_MFMA) eat the reference fixture: image
    A_K5_D2, the fixture's six minibatches of 96 rows as three "epochs" of two (perm = the two batches, bs = 96),
    the fixture's StepLR chain -- same 1e-5 bounds on loss and parameters as the generic step meets below."""
    T = golden["train"]
    F = golden["features"]
    img, K, D = F["A_K5_D2/img"], 5, 2
    C, H, W = img.shape
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, FeatCfg(), dev)
    net = ops.make_net(200, 64, 8, 2)
    p = torch.from_numpy(T["params0"].copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = ops.TrainWorkspace(geom, net, 96, dev).prepare(img_d, msb_d, ops._lib.PATH_MFMA)
    for e in range(3):
        perm = torch.from_numpy(np.concatenate([T["batches"][2 * e], T["batches"][2 * e + 1]])).to(dev)
        assert float(T[f"step{2 * e}/lr"]) == float(T[f"step{2 * e + 1}/lr"])
        losses = torch.zeros(2, dtype=torch.float32, device=dev)
        ops.train_epoch(geom, net, img_d, msb_d, perm, 96, p, m, v, 2 * e, float(T[f"step{2 * e}/lr"]), losses,
                        ops._lib.PATH_MFMA, ws, alone=alone)
        for k in range(2):
            ref = float(T[f"step{2 * e + k}/loss"])
            assert abs(float(losses[k].item()) - ref) <= RTOL_TRAIN * ref, (e, k)
        pr = T[f"step{2 * e + 1}/params"]
        assert np.linalg.norm(p.cpu().numpy() - pr) <= 1e-5 * np.linalg.norm(pr), e
    np.testing.assert_allclose(m.cpu().numpy(), T["exp_avg"], rtol=0, atol=1e-5 * np.abs(T["exp_avg"]).max())
    np.testing.assert_allclose(v.cpu().numpy(), T["exp_avg_sq"], rtol=0, atol=1e-5 * np.abs(T["exp_avg_sq"]).max())



# ---------------------------------------------------------------- the reference's majority shape: 4 bands, F = 100

def test_bands4_features_and_forward_match_reference_fixture(golden, dev):
    """C = 4, K5 D2, relative colours (9 of the 13 images of the reference's run.sh:14-28): the HIP feature / label kernels
    give the bits of the reference's process(), the HIP forward is bit-exact vs the oracle and within 1e-5 of the
    reference's LBDRNModel(100, 64, 4, 2) at the seeded initial weights and at a copy whose sines wrap."""
    G = golden["bands4"]
    img = G["small/img"]
    C, H, W = img.shape
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, 5)
    geom = ops.FeatureGeometry(C, H, W, 5, 2, mx, FeatCfg(), dev)
    f = ops.features(geom, msb_d).cpu().numpy()
    assert np.array_equal(_bits(f), _bits(G["small/features"]))
    assert np.array_equal(_bits(ops.labels(img_d, 5).cpu().numpy()), _bits(G["small/labels"]))
    net = ops.make_net(100, 64, 4, 2)
    for case in ("init", "wide"):
        p = G[f"small/{case}_params"]
        y = ops.forward(net, torch.from_numpy(p).to(dev), torch.from_numpy(G["small/features"]).to(dev)).cpu().numpy()
        assert np.array_equal(_bits(y), _bits(O.forward(p, 100, 64, 4, 2, G["small/features"])))
        np.testing.assert_allclose(y, G[f"small/{case}_y"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("alone", (False, True))
@pytest.mark.parametrize("tag,rows", (("small", 96), ("ragged", 200)))
def test_bands4_train_kernels_match_reference_fixture(golden, dev, tag, rows, alone):
    """The fused steps of the 4-band shape -- k_train_stream<24, 2, 3, 6> and, with the hint of a lone fit,
    k_train_split<24, 6> (96 executed features: six strips, one per wave and two left over) -- eat reference fixtures of
    their own: six teacher-forced updates with the StepLR chain, minibatches of 96 rows (one and a half 64-row groups) and
    of 200 (three groups and eight rows: one parity of the last pair of workgroups nearly empty).  Loss 1e-5 per step,
    parameters 2e-5, Adam moments as close to the float64 evaluation of the same steps as the reference's run is."""
    G = golden["bands4"]
    img = G[tag + "/img"]
    lrs = [float(G[f"{tag}/step{s}/lr"]) for s in range(6)]
    batches = list(G[tag + "/batches"])
    assert len(batches[0]) == rows
    p, m, v = _fused_steps_vs_fixture(dev, img, FeatCfg(), 64, G[tag + "/params0"], batches, lrs,
                                      [G[f"{tag}/step{s}/loss"] for s in range(6)], rows, alone=alone)
    pr = G[f"{tag}/step5/params"]
    msb, lab, mx = O.split_bits(img, 5)
    feats = O.features(msb, 2, O.FeatCfg(), mx)
    p64, m64, v64 = _f64_steps(feats, lab, G[tag + "/params0"], batches, 100, 64, 4, lrs)
    # (Adam's first steps move every parameter by ~lr * sign(g): where a gradient is near zero its rounding decides the
    #  direction -- measured 1.26e-5 on "ragged" --, so the vector is held to 2e-5 of the reference run, as at bc = 256, and to
    #  being as close to the float64 evaluation of the same six steps as the reference's own float32 run is, x2)
    assert np.linalg.norm(p - pr) <= 2e-5 * np.linalg.norm(pr)
    assert np.linalg.norm(p - p64) <= 2 * np.linalg.norm(pr - p64) + 1e-6 * np.linalg.norm(p64)
    _as_close_to_float64_as_the_reference("exp_avg", m, G[tag + "/exp_avg"], m64)
    _as_close_to_float64_as_the_reference("exp_avg_sq", v, G[tag + "/exp_avg_sq"], v64)


def test_bands4_learnable_raster_hip_oracle_reference(golden, dev):
    """A reference-made 4 x 256 x 256 raster from a fit that learns (tests/golden/make_golden_bands4.py): HIP == oracle bit
    for bit on every path; HIP differs from the reference raster only at listed near-boundary sub-pixels."""
    G = golden["rasters_learn_bands4"]
    img, K, D, bc, nl = G["img"], int(G["K"]), int(G["D"]), int(G["bc"]), int(G["nl"])
    cfg = _cfg(G["flags"])
    msb, _, mx = O.split_bits(img, K)
    C, H, W = img.shape
    assert C == 4
    out_o = O.decode(msb, K, D, _ocfg(cfg), G["params"], bc, nl, mx)
    ref = ((img >> K) << K) + G["residual"]
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(cfg.feature_dim(C, D), bc, C, nl)
    p_d, msb_d = torch.from_numpy(G["params"]).to(dev), ops.to_device_u16(msb, dev)
    for path in (ops._lib.PATH_GENERIC, ops._lib.PATH_AUTO, ops._lib.PATH_MFMA):
        out = ops.from_device_u16(ops.decode_fused(geom, net, msb_d, p_d, path=path))
        assert np.array_equal(out, out_o), path
        bad = np.flatnonzero((out != ref).transpose(1, 2, 0).reshape(-1))
        assert np.isin(bad, G["near_idx"]).all(), path
        assert bad.size <= 2


def test_train_steps_match_reference_fixture(golden, dev):
    """Teacher-forced updates vs torch autograd + torch.optim.Adam + StepLR run on the reference's
    model/loss (tests/golden/make_golden.py): loss within 1e-5 relative at every step."""
    T = golden["train"]
    net = ops.make_net(200, 64, 8, 2)
    p = torch.from_numpy(T["params0"].copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    x, t = torch.from_numpy(T["x"]).to(dev), torch.from_numpy(T["t"]).to(dev)
    for s in range(6):
        b = torch.from_numpy(T["batches"][s]).to(dev)
        loss, g = ops.train_step(net, x[b], t[b], p, m, v, s + 1, float(T[f"step{s}/lr"]))
        ref = float(T[f"step{s}/loss"])
        assert abs(float(loss.item()) - ref) <= RTOL_TRAIN * ref
        gr = T[f"step{s}/grads"]
        assert np.linalg.norm(g.cpu().numpy() - gr) <= 1e-5 * np.linalg.norm(gr)
        pr = T[f"step{s}/params"]
        assert np.linalg.norm(p.cpu().numpy() - pr) <= 1e-5 * np.linalg.norm(pr)
    np.testing.assert_allclose(m.cpu().numpy(), T["exp_avg"], rtol=0, atol=1e-5 * np.abs(T["exp_avg"]).max())
    np.testing.assert_allclose(v.cpu().numpy(), T["exp_avg_sq"], rtol=0, atol=1e-5 * np.abs(T["exp_avg_sq"]).max())


def test_other_widths_match_reference_fixture(golden, dev):
    """bc=256 (BASELINE configs[2]) and nl in {1, 3}: HIP forward within 3e-6 of the reference model's, and
    three teacher-forced bc=256 updates within the training tolerance of torch autograd + Adam."""
    G = golden["wide_net"]
    x, t = torch.from_numpy(G["x"]).to(dev), torch.from_numpy(G["t"]).to(dev)
    for tag, bc, nl in (("bc256_nl2", 256, 2), ("bc64_nl3", 64, 3), ("bc128_nl1", 128, 1)):
        y = ops.forward(ops.make_net(200, bc, 8, nl), torch.from_numpy(G[tag + "/params"]).to(dev), x)
        np.testing.assert_allclose(y.cpu().numpy(), G[tag + "/y"], rtol=3e-6, atol=3e-7)
    net = ops.make_net(200, 256, 8, 2)
    p = torch.from_numpy(G["train256/params0"].copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for s in range(3):
        b = torch.from_numpy(G["train256/batches"][s]).to(dev)
        loss, g = ops.train_step(net, x[b], t[b], p, m, v, s + 1, 1e-3)
        ref = float(G[f"train256/step{s}/loss"])
        assert abs(float(loss.item()) - ref) <= RTOL_TRAIN * ref
        if s == 0:
            gr = G["train256/step0/grads"]
            assert np.linalg.norm(g.cpu().numpy() - gr) <= 1e-5 * np.linalg.norm(gr)
    pr = G["train256/params_final"]
    assert np.linalg.norm(p.cpu().numpy() - pr) <= 2e-5 * np.linalg.norm(pr)


@pytest.mark.parametrize("F,bc,C,nl,B", [(200, 64, 8, 2, 300), (18, 16, 3, 3, 64), (27, 32, 3, 1, 1000),
                                         (200, 256, 8, 2, 257)])  # last: BASELINE config 3 shape
def test_train_step_vs_oracle(dev, F, bc, C, nl, B):
    rng = np.random.default_rng(B + F)
    p0 = _rand_params(rng, F, bc, C, nl)
    x = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    t = rng.integers(0, 32, (B, C)).astype(np.float32) / 31
    po, mo, vo = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    p = torch.from_numpy(p0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    net = ops.make_net(F, bc, C, nl)
    for s in range(3):
        lo, go = O.train_step(po, mo, vo, F, bc, C, nl, x, t, 1e-3, s + 1)
        loss, g = ops.train_step(net, torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev), p, m, v, s + 1, 1e-3)
        assert abs(float(loss.item()) - lo) <= RTOL_TRAIN * lo
        assert np.linalg.norm(g.cpu().numpy() - go) <= 2e-5 * np.linalg.norm(go)
        assert np.linalg.norm(p.cpu().numpy() - po) <= 1e-5 * np.linalg.norm(po)


def test_train_epoch_vs_oracle_sequence(dev):
    """lbdrn_train_epoch (gather by permutation + update, short last batch) against the oracle run
    step by step on oracle features/labels."""
    rng = np.random.default_rng(5)
    C, H, W, K, D, bc, nl, bs = 4, 23, 31, 5, 2, 64, 2, 200
    cfg = FeatCfg()
    img = _image(rng, C, H, W)
    msb, lab, mx = O.split_bits(img, K)
    feats = O.features(msb, D, _ocfg(cfg), mx)
    F = feats.shape[1]
    p0 = _rand_params(rng, F, bc, C, nl)
    perm = rng.permutation(H * W).astype(np.int64)
    po, mo, vo = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    losses_o = []
    nsteps = (H * W + bs - 1) // bs
    for s in range(nsteps):
        b = perm[s * bs:(s + 1) * bs]
        lo, _ = O.train_step(po, mo, vo, F, bc, C, nl, feats[b], lab[b], 1e-3, 7 + s + 1)
        losses_o.append(lo)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(F, bc, C, nl)
    p = torch.from_numpy(p0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(nsteps, dtype=torch.float32, device=dev)
    ops.train_epoch(geom, net, ops.to_device_u16(img, dev), ops.to_device_u16(msb, dev),
                    torch.from_numpy(perm).to(dev), bs, p, m, v, 7, 1e-3, losses)
    np.testing.assert_allclose(losses.cpu().numpy(), np.array(losses_o), rtol=RTOL_TRAIN)
    assert np.linalg.norm(p.cpu().numpy() - po) <= 1e-5 * np.linalg.norm(po)


def test_train_epoch_is_bitwise_reproducible(dev):
    rng = np.random.default_rng(9)
    C, H, W, K, D, bc, nl, bs = 8, 40, 48, 5, 2, 64, 2, 512
    img = _image(rng, C, H, W)
    msb, _, mx = O.split_bits(img, K)
    F = 200
    p0 = _rand_params(rng, F, bc, C, nl)
    perm = torch.from_numpy(rng.permutation(H * W).astype(np.int64)).to(dev)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, FeatCfg(), dev)
    net = ops.make_net(F, bc, C, nl)
    outs = []
    for _ in range(2):
        p = torch.from_numpy(p0.copy()).to(dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        ops.train_epoch(geom, net, ops.to_device_u16(img, dev), ops.to_device_u16(msb, dev), perm, bs, p, m, v, 0, 1e-3)
        outs.append(p.cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_drop_in_process_and_dataset_equal_reference_fixture(golden, dev, tmp_path, monkeypatch):
    """The drop-in LBDRNdataset.process() / LBDRNDataset (the reference's own entry points, ref
    LBDRNdataset.py:92-155) on every fixture case: feature and label matrices bit-identical to what the
    reference's process() returned, the written MSB raster is img >> K with the reference's dtype rule, and
    the Dataset exposes the same attributes and items."""
    import argparse
    import constants
    import LBDRNdataset as DS
    from lbdrn_hip import raster_io
    G = golden["features"]
    names = sorted({k.split("/")[0] for k in G.files})
    assert len(names) >= 10
    for name in names:
        img, K, D = G[name + "/img"], int(G[name + "/K"]), int(G[name + "/D"])
        for flag, val in zip(("USE_COORDINATES", "EMBEDDING", "USE_COLORS", "RELATIVE"), G[name + "/flags"]):
            monkeypatch.setattr(constants, flag, bool(val))
        src = str(tmp_path / f"{name}.npy")
        np.save(src, img)
        f, l = DS.process(src, K, D, str(tmp_path / f"{name}_base.tif"))
        assert f.dtype == np.float32 and np.array_equal(f.view(np.int32), G[name + "/features"].view(np.int32)), name
        assert np.array_equal(l.view(np.int32), G[name + "/labels"].view(np.int32)), name
        base = raster_io.read_raster(str(tmp_path / f"{name}_base.tif")).reshape(img.shape)
        assert np.array_equal(base, img >> K), name
        assert base.dtype == (np.uint16 if int((img >> K).max()) > 255 else np.uint8), name   # LBDRNdataset.py:100
        ds = DS.LBDRNDataset(argparse.Namespace(path=src, output_dir=str(tmp_path), K=K, D=D))
        assert (ds.n_pixels, ds.n_feature, ds.channels, ds.n_subpixels) == \
            (f.shape[0], f.shape[1], l.shape[1], f.shape[0] * l.shape[1]), name
        assert len(ds) == f.shape[0]
        x7, t7 = ds[min(7, len(ds) - 1)]
        assert torch.equal(x7, torch.from_numpy(f[min(7, len(ds) - 1)])) and t7.dtype == torch.float32
