"""torch.autograd on the drop-in LBDRNModel (lbdrn_forward_tape / lbdrn_backward behind lbdrn_hip.autograd): the
reference's own trainer step (modified_ignite_engine.py:18-27) on the reference's fixtures, bit-identity with the
fused-loss generic step, arbitrary upstream gradients against a float64 restatement, autograd semantics, and the
INTEGRATION.md example."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from lbdrn_hip import ops, sampler
from lbdrn_hip.autograd import split_flat
from lbdrn_hip.features import FeatCfg
from lbdrn_hip.model import LBDRNLoss, LBDRNModel
from train_step_f64 import f64_steps

pytestmark = pytest.mark.gpu

RTOL_TRAIN = 1e-5   # as test_gpu_parity.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nrel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


def _model(dev, F, bc, C, nl, params0=None, relu=False):
    m = LBDRNModel(F, bc, C, nl, activation=nn.ReLU() if relu else None).to(dev)
    if params0 is not None:
        ps = m.hip_parameters()
        with torch.no_grad():
            for p, v in zip(ps, split_flat(torch.from_numpy(np.asarray(params0, np.float32)), [p.shape for p in ps])):
                p.copy_(v)
    return m


def _flat_grad(model):
    return torch.cat([p.grad.reshape(-1) for p in model.hip_parameters()]).cpu().numpy()


def _reference_loop(dev, model, X, T, batches, lrs):
    """The reference's trainer: Adam(model.parameters(), lr), the StepLR chain as per-step lr, and the `_update` body
    verbatim.  Returns per step (loss, flat p.grad, flat params) and the optimizer."""
    optimizer = torch.optim.Adam(model.parameters(), lr=lrs[0])
    loss_fn = LBDRNLoss()
    device, non_blocking = dev, False

    def prepare_batch(batch, device=None, non_blocking=False):
        x, y = batch
        return x.to(device, non_blocking=non_blocking), y.to(device, non_blocking=non_blocking)

    def _update(engine, batch):
        optimizer.zero_grad()
        model.train()
        x, y = prepare_batch(batch, device=device, non_blocking=non_blocking)
        y_pred = model(x)
        loss = loss_fn(y_pred, y)
        loss.backward()
        optimizer.step()

        return loss

    out = []
    for s, b in enumerate(batches):
        for g in optimizer.param_groups:
            g["lr"] = float(lrs[s])
        b = torch.from_numpy(np.asarray(b))
        loss = _update(None, (X[b], T[b]))
        out.append((float(loss.item()), _flat_grad(model), model.flat_parameters().cpu().numpy()))
    return out, optimizer


def _moments(model, optimizer):
    st = [optimizer.state[p] for p in model.hip_parameters()]
    return (torch.cat([s["exp_avg"].reshape(-1) for s in st]).cpu().numpy(),
            torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).cpu().numpy())


def _f64_steps(x, t, params0, batches, F, bc, C, lrs):
    """Teacher-forced Sine nl = 2 updates in float64 numpy (tests/train_step_f64.py): exact arithmetic, to tell the
    run's rounding from the reference run's own where the fixture's Adam moments are held to that."""
    return f64_steps(x, t, params0, batches, F, bc, C, lrs, act="sine", nl=2)


def _as_close_to_float64_as_the_reference(name, run, ref32, ref64):
    scale = np.abs(ref64).max()
    err_ref, err_run = np.abs(ref32 - ref64).max() / scale, np.abs(run - ref64).max() / scale
    assert err_run <= max(1e-5, 2 * err_ref), (name, err_run, err_ref)


def _device_features(dev, img, cfg, K=5, D=2):
    C, H, W = img.shape
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx = ops.split_bits(img_d, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    return ops.features(geom, msb_d).cpu(), ops.labels(img_d, K).cpu()


def _cases(golden, dev):
    """(name, F, bc, C, nl, relu, X, T, params0, batches, lrs, fixture arrays by key prefix, params bound)"""
    T = golden["train"]
    yield ("train", 200, 64, 8, 2, False, T["x"], T["t"], T["params0"], list(T["batches"]),
           [float(T[f"step{s}/lr"]) for s in range(6)], lambda k: T[k] if k in T else None, 1e-5)
    R = golden["relu_net"]
    # (params: 2e-5, the bound test_gpu_relu.py holds the generic step's final parameters of this fixture to)
    yield ("relu", 200, 64, 8, 2, True, R["x"], R["t"], R["train/params0"], list(R["train/batches"]), [1e-3] * 3,
           lambda k: R["train/" + k] if "train/" + k in R else None, 2e-5)
    Wd = golden["wide_net"]
    yield ("train256", 200, 256, 8, 2, False, Wd["x"], Wd["t"], Wd["train256/params0"], list(Wd["train256/batches"]),
           [1e-3] * 3, lambda k: Wd["train256/" + k] if "train256/" + k in Wd else None, 2e-5)
    B4 = golden["bands4"]
    yield ("bands4/small", 100, 64, 4, 2, False, B4["small/features"], B4["small/labels"], B4["small/params0"],
           list(B4["small/batches"]), [float(B4[f"small/step{s}/lr"]) for s in range(6)],
           lambda k: B4["small/" + k] if "small/" + k in B4 else None, 2e-5)
    Xr, Tr = _device_features(dev, B4["ragged/img"], FeatCfg())
    yield ("bands4/ragged", 100, 64, 4, 2, False, Xr, Tr, B4["ragged/params0"], list(B4["ragged/batches"]),
           [float(B4[f"ragged/step{s}/lr"]) for s in range(6)],
           lambda k: B4["ragged/" + k] if "ragged/" + k in B4 else None, 2e-5)
    E = golden["train2"]
    f = E["embed/flags"]
    cfg = FeatCfg(use_coordinates=bool(f[0]), embedding=bool(f[1]), use_colors=bool(f[2]), relative=bool(f[3]))
    Xe, Te = _device_features(dev, E["embed/img"], cfg)
    yield ("embed", 250, 64, 8, 2, False, Xe, Te, E["embed/params0"], list(E["embed/batches"]),
           [float(E[f"embed/step{s}/lr"]) for s in range(6)],
           lambda k: E["embed/" + k] if "embed/" + k in E else None, 1e-5)


CASES = ("train", "relu", "train256", "bands4/small", "bands4/ragged", "embed")


@pytest.mark.parametrize("case", CASES)
def test_reference_trainer_step_eats_the_reference_fixtures(golden, dev, case):
    """The `_update` body verbatim (zero_grad, train(), forward, LBDRNLoss, backward(), Adam.step) on LBDRNModel loaded
    with the fixture's params0: loss 1e-5 relative every step, p.grad 1e-5 norm-relative wherever the fixture has
    gradients, parameters at the fixture's bound, Adam moments from optimizer.state at the existing bounds."""
    name, F, bc, C, nl, relu, X, T, p0, batches, lrs, fx, pbound = next(c for c in _cases(golden, dev) if c[0] == case)
    X = torch.as_tensor(np.asarray(X, np.float32))
    T = torch.as_tensor(np.asarray(T, np.float32))
    model = _model(dev, F, bc, C, nl, p0, relu)
    out, optimizer = _reference_loop(dev, model, X, T, batches, lrs)
    for s, (loss, grad, params) in enumerate(out):
        ref = float(fx(f"step{s}/loss"))
        assert abs(loss - ref) <= RTOL_TRAIN * ref, (s, loss, ref)
        gr = fx(f"step{s}/grads")
        if gr is not None:
            assert _nrel(grad, gr) <= 1e-5, (s, _nrel(grad, gr))
        pr = fx(f"step{s}/params")
        if pr is not None:
            assert _nrel(params, pr) <= pbound, (s, _nrel(params, pr))
    pr = fx("params_final")
    if pr is not None:
        assert _nrel(out[-1][2], pr) <= pbound, _nrel(out[-1][2], pr)
    m, v = _moments(model, optimizer)
    if case == "train":
        np.testing.assert_allclose(m, fx("exp_avg"), rtol=0, atol=1e-5 * np.abs(fx("exp_avg")).max())
        np.testing.assert_allclose(v, fx("exp_avg_sq"), rtol=0, atol=1e-5 * np.abs(fx("exp_avg_sq")).max())
    elif fx("exp_avg") is not None or case == "train256":
        ref_m = fx("exp_avg") if case != "train256" else golden["train2"]["wide256/exp_avg"]
        ref_v = fx("exp_avg_sq") if case != "train256" else golden["train2"]["wide256/exp_avg_sq"]
        p64, m64, v64 = _f64_steps(X.numpy(), T.numpy(), np.asarray(p0), batches, F, bc, C, lrs)
        _as_close_to_float64_as_the_reference("exp_avg", m, ref_m, m64)
        _as_close_to_float64_as_the_reference("exp_avg_sq", v, ref_v, v64)


def _rand_params(rng, F, bc, C, nl):
    parts = []
    for l in range(nl):
        nin = F if l == 0 else bc
        b = 1.0 / nin if l == 0 else np.sqrt(6.0 / nin) / 30.0
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize("F,bc,C,nl,B,relu", [(200, 64, 8, 2, 300, False), (18, 16, 3, 3, 64, False),
                                              (27, 32, 3, 1, 1000, False), (200, 256, 8, 2, 257, False),
                                              (200, 64, 8, 2, 300, True)])
def test_backward_of_the_mse_gradient_is_the_fused_loss_steps_bit_for_bit(dev, F, bc, C, nl, B, relu):
    """lbdrn_backward fed dy = (2 (y - t)) / (B C), formed in float32 as k_loss_grad forms it, gives lbdrn_train_step's
    grads bit for bit; the tape's y is lbdrn_forward's bit for bit."""
    rng = np.random.default_rng(B + F + nl)
    p0 = _rand_params(rng, F, bc, C, nl)
    x = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    t = (rng.integers(0, 32, (B, C)).astype(np.float32) / 31).astype(np.float32)
    net = ops.make_net(F, bc, C, nl, ops.ACT_RELU if relu else ops.ACT_SINE)
    p, xd, td = (torch.from_numpy(a).to(dev) for a in (p0, x, t))
    y, tape = ops.forward_tape(net, p, xd)
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(ops.forward(net, p, xd).cpu().numpy()))
    yh = y.cpu().numpy()
    inv = np.float32(1) / (np.float32(B) * np.float32(C))
    dy = (np.float32(2) * (yh - t)) * inv
    assert dy.dtype == np.float32
    grads, dx = ops.backward(net, p, xd, tape, y, torch.from_numpy(dy).to(dev))
    assert dx is None
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    _, g_ref = ops.train_step(net, xd, td, p, m, v, 1, 1e-3, apply_adam=False)
    assert np.array_equal(_bits(grads.cpu().numpy()), _bits(g_ref.cpu().numpy()))
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(p0))       # apply_adam=0 left the parameters alone


def _restated(params, x, F, bc, C, nl, relu):
    """LBDRNModel in float64 torch on the CPU: Linear + sin(30 z) / ReLU hidden layers, Linear + sigmoid head."""
    h, o = x, 0
    for l in range(nl):
        nin = F if l == 0 else bc
        W = params[o:o + bc * nin].view(bc, nin); o += bc * nin
        b = params[o:o + bc]; o += bc
        z = h @ W.T + b
        h = torch.relu(z) if relu else torch.sin(30 * z)
    W = params[o:o + C * bc].view(C, bc); o += C * bc
    return torch.sigmoid(h @ W.T + params[o:o + C])


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("nl", (1, 3))
def test_arbitrary_upstream_gradient_and_input_gradient_vs_float64(dev, nl, relu):
    """A random dL/dy (not an MSE gradient) and x.requires_grad_(): p.grad and x.grad within 2e-5 norm-relative of a
    float64 CPU autograd restatement of the same network."""
    F, bc, C, B = 50, 48, 5, 700
    torch.manual_seed(11 + nl)
    model = _model(dev, F, bc, C, nl, relu=relu)
    rng = np.random.default_rng(nl + 10 * relu)
    x0 = rng.uniform(-1, 1, (B, F)).astype(np.float32)
    dy = rng.standard_normal((B, C)).astype(np.float32)
    x = torch.from_numpy(x0).to(dev).requires_grad_()
    model.train()
    y = model(x)
    assert y.grad_fn is not None
    (y * torch.from_numpy(dy).to(dev)).sum().backward()
    p64 = model.flat_parameters().cpu().double().requires_grad_()
    x64 = torch.from_numpy(x0).double().requires_grad_()
    y64 = _restated(p64, x64, F, bc, C, nl, relu)
    (y64 * torch.from_numpy(dy).double()).sum().backward()
    assert _nrel(_flat_grad(model), p64.grad.numpy()) <= 2e-5
    assert _nrel(x.grad.cpu().numpy(), x64.grad.numpy()) <= 2e-5
    assert np.abs(y.detach().cpu().numpy() - y64.detach().numpy()).max() <= 1e-5


def test_autograd_semantics(dev):
    F, bc, C, nl, B = 40, 32, 3, 2, 200
    torch.manual_seed(5)
    model = _model(dev, F, bc, C, nl)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, F)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rng.uniform(0, 1, (B, C)).astype(np.float32)).to(dev)
    loss_fn = LBDRNLoss()
    # a fresh module (training by default, never told train()), eval(), and no_grad() after train(): no graph
    assert model(x).grad_fn is None
    assert model(x).cpu().numpy().shape == (B, C)
    model.eval()
    assert model(x).grad_fn is None
    model.train()
    with torch.no_grad():
        assert model(x).grad_fn is None
    # two passes without zero_grad accumulate: exactly twice one pass
    loss_fn(model(x), t).backward()
    g1 = [p.grad.clone() for p in model.hip_parameters()]
    assert model.hip_parameters()[0].grad is not None
    loss_fn(model(x), t).backward()
    for p, g in zip(model.hip_parameters(), g1):
        assert torch.equal(p.grad, 2 * g)
    # a frozen layer keeps .grad None; the others get the same gradients as before
    model.zero_grad(set_to_none=True)
    first = model.net[0].linear
    first.weight.requires_grad_(False)
    first.bias.requires_grad_(False)
    loss_fn(model(x), t).backward()
    assert first.weight.grad is None and first.bias.grad is None
    for p, g in zip(model.hip_parameters()[2:], g1[2:]):
        assert torch.equal(p.grad, g)
    # x requiring grad alone records too
    model.zero_grad(set_to_none=True)
    for p in model.parameters():
        p.requires_grad_(False)
    xg = x.clone().requires_grad_()
    assert model(xg).grad_fn is not None
    for p in model.parameters():
        p.requires_grad_(True)
    # parameters on another device than x: raises, nothing is copied
    cpu_model = _model(torch.device("cpu"), F, bc, C, nl)
    cpu_model.train()
    with pytest.raises(ops._lib.LbdrnError):
        cpu_model(x)


def _integration_example():
    s = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hit = [b for b in re.findall(r"```python\n(.*?)```", s, re.S) if "def _update(engine, batch):" in b]
    assert len(hit) == 1, "INTEGRATION.md lost its autograd training example"
    return hit[0]


def test_integration_example_runs_one_epoch_like_the_generic_step(dev, tmp_path, monkeypatch):
    """The INTEGRATION.md autograd example, verbatim, on a synthetic tile through the drop-in LBDRNDataset: its minibatch
    order is the permutation lbdrn_hip.sampler predicts for that DataLoader, and its per-step losses are within 1e-4
    relative of the generic ops.train_step driven with the same batches."""
    import LBDRNdataset
    from lbdrn_hip import raster_io
    from lbdrn_hip.synth import synthetic_tile
    C, H, W, K, D, bc, nl, bs, lr, seed = 8, 36, 44, 5, 2, 64, 2, 256, 1e-3, 1234
    img = synthetic_tile(3, C, H, W)
    path = str(tmp_path / "tile.tif")
    raster_io.write_raster(path, img)

    class Args:
        pass
    args = Args()
    args.path, args.K, args.D, args.output_dir = path, K, D, str(tmp_path)
    args.batch_size, args.base_channel, args.num_layers, args.lr = bs, bc, nl, lr
    seen = []
    get = LBDRNdataset.LBDRNDataset.__getitem__
    monkeypatch.setattr(LBDRNdataset.LBDRNDataset, "__getitem__", lambda self, i: (seen.append(int(i)), get(self, i))[1])
    torch.manual_seed(seed)
    env = {"args": args}
    exec(compile(_integration_example(), "INTEGRATION.md:autograd", "exec"), env)
    torch.cuda.synchronize()
    n = H * W
    F = C * (2 * D + 1) ** 2
    # the order: the model's initialisation draws first, then the DataLoader iterator's two draws
    torch.manual_seed(seed)
    p0 = LBDRNModel(F, bc, C, nl).flat_parameters()
    perm = sampler.permutation(sampler.draw_iterator_seed(), n)
    assert seen == perm.tolist()
    # the generic fused-loss step on the same batches
    ds = env["dataset"]
    net = ops.make_net(F, bc, C, nl)
    p = p0.to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    want = []
    for s, first in enumerate(range(0, n, bs)):
        b = perm[first:first + bs]
        loss, _ = ops.train_step(net, ds.features[b].to(dev), ds.labels[b].to(dev), p, m, v, s + 1, lr)
        want.append(float(loss.item()))
    got = env["epoch_losses"]
    assert len(got) == len(want)
    rel = [abs(a - b) / b for a, b in zip(got, want)]
    assert max(rel) <= 1e-4, rel
