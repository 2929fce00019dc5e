"""The generic training step and the autograd backward (csrc/generic.hip) against the ordered float32 restatement of the
oracle (oracle/lbdrn_oracle.c: orc_step_ordered), bit for bit: loss, every gradient, both Adam moments, the parameters, y
and dL/dx.  The generic step is what every fused training kernel is held to, and the only step of the shapes they refuse;
its order is a contract (generic.hip's header), so there is no tolerance anywhere in this file.

The shapes are the fixed table of tests/generic_step_rows.py, one row per tile, slice and reduce-loop edge;
tests/test_generic_step_ordered_host.py shows on the CPU that the restatement is a training step, that every row's inputs
tell the kernels' order from its neighbours', and that no row leaves the normal float32 range."""
import ctypes

import numpy as np
import pytest
import torch

import oracle as O
from generic_step_rows import BY_NAME, LR, ROWS, first_step, init_params, inputs, ordered_step
from guarded import Arena
from lbdrn_hip import _lib, ops
from lbdrn_hip.features import FeatCfg
from train_plan_reference import BS, BS_TAIL, H, K, W

pytestmark = pytest.mark.gpu
GEN = _lib.PATH_GENERIC


def _same(got, want):
    """bit equality of two float32 arrays (a tensor is fetched first)"""
    if isinstance(got, torch.Tensor):
        got = got.cpu().numpy()
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _differing(got, want):
    got = np.ascontiguousarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, np.float32).reshape(-1)
    bad = np.flatnonzero(got.view(np.int32) != np.ascontiguousarray(want, np.float32).reshape(-1).view(np.int32))
    return f"{bad.size} of {got.size} entries differ, first at {bad[:4].tolist()}"


def _act(row):
    return ops.ACT_RELU if row.act == "relu" else ops.ACT_SINE


def _net(row):
    return ops.make_net(row.F, row.bc, row.C, row.nl, _act(row))


def _assert_state(got, want, what):
    for k in ("loss", "grads", "exp_avg", "exp_avg_sq", "params"):
        assert _same(np.reshape(got[k], -1), np.reshape(want[k], -1)), (what, k, _differing(got[k], np.reshape(want[k], -1)))


# ------------------------------------------------------------------ (a) one step, every gradient

@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_one_step_equals_the_ordered_oracle(dev, row):
    p0, x, t, _ = inputs(row)
    p, xd, td = (torch.from_numpy(a.copy()).to(dev) for a in (p0, x, t))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    loss, grads = ops.train_step(_net(row), xd, td, p, m, v, 1, LR)
    got = dict(loss=loss.cpu().numpy(), grads=grads.cpu().numpy(), exp_avg=m.cpu().numpy(), exp_avg_sq=v.cpu().numpy(),
               params=p.cpu().numpy())
    _assert_state(got, first_step(row), row.name)


# ------------------------------------------------------------------ (b) three steps

@pytest.mark.parametrize("first", (1, 1000), ids=lambda s: f"from_step{s}")
@pytest.mark.parametrize("name", ("T1", "T4", "T9"))
def test_three_steps_equal_the_ordered_oracle(dev, name, first):
    """Adam on nonzero moments, at step counts 1..3 and at 1000..1002 (bias corrections far from their first values)."""
    row = BY_NAME[name]
    p0, x, t, _ = inputs(row)
    p, xd, td = (torch.from_numpy(a.copy()).to(dev) for a in (p0, x, t))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    state = (p0.copy(), np.zeros_like(p0), np.zeros_like(p0))
    for step in range(first, first + 3):
        loss, grads = ops.train_step(_net(row), xd, td, p, m, v, step, LR)
        want = ordered_step(row, step=step, state=state)
        state = (want["params"], want["exp_avg"], want["exp_avg_sq"])
        got = dict(loss=loss.cpu().numpy(), grads=grads.cpu().numpy(), exp_avg=m.cpu().numpy(), exp_avg_sq=v.cpu().numpy(),
                   params=p.cpu().numpy())
        _assert_state(got, want, (name, step))


# ------------------------------------------------------------------ (c) an epoch under PATH_GENERIC

EPOCH_SHAPES = {"C4_D2_bc64_nl2_sine": (4, 2, 64, 2, "sine"),
                "C3_D1_bc96_nl3_relu": (3, 1, 96, 3, "relu")}   # bc = 96: a shape only the generic path serves


@pytest.mark.parametrize("bs", (BS, BS_TAIL), ids=lambda b: f"bs{b}")
@pytest.mark.parametrize("shape", sorted(EPOCH_SHAPES))
def test_two_epochs_equal_the_ordered_oracle(dev, shape, bs):
    """lbdrn_train_epoch(PATH_GENERIC) on the 13 x 11 raster: minibatches of 100 and 43, or of 71, 71 and 1; losses,
    parameters and moments after two epochs (the second numbering its steps on from the first)."""
    C, D, bc, nl, act = EPOCH_SHAPES[shape]
    rng = np.random.default_rng([C, D, bc, nl, bs])
    img = rng.integers(0, 1 << 9, (C, H, W)).astype(np.uint16)
    img[0, 0, 0] |= np.uint16(1 << K)
    cfg = FeatCfg(activation=act)
    F = cfg.feature_dim(C, D)
    p0 = init_params(rng, F, bc, C, nl, act)
    perms = [rng.permutation(H * W).astype(np.int64) for _ in range(2)]
    nsteps = (H * W + bs - 1) // bs
    assert [min(bs, H * W - f) for f in range(0, H * W, bs)] == ([100, 43] if bs == BS else [71, 71, 1])

    msb, _, mx = O.split_bits(img, K)
    geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
    net = ops.make_net(F, bc, C, nl, cfg.act)
    img_d, msb_d = ops.to_device_u16(img, dev), ops.to_device_u16(msb, dev)
    p = torch.from_numpy(p0.copy()).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    losses = torch.zeros(2 * nsteps, dtype=torch.float32, device=dev)
    ws = ops.TrainWorkspace(geom, net, bs, dev).prepare(img_d, msb_d, GEN)
    for e, perm in enumerate(perms):
        ops.train_epoch(geom, net, img_d, msb_d, torch.from_numpy(perm).to(dev), bs, p, m, v, e * nsteps, LR,
                        losses[e * nsteps:(e + 1) * nsteps], path=GEN, ws=ws)

    po, mo, vo = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    ocfg = O.FeatCfg(cfg.use_coordinates, cfg.embedding, cfg.sigma, cfg.n_freq, cfg.use_colors, cfg.relative)
    with O.hidden_activation(act):
        lo = np.concatenate([O.train_epoch_ordered(img, K, D, ocfg, po, mo, vo, bc, nl, perm, bs, LR, e * nsteps)
                             for e, perm in enumerate(perms)])
    got = dict(loss=losses.cpu().numpy(), exp_avg=m.cpu().numpy(), exp_avg_sq=v.cpu().numpy(), params=p.cpu().numpy())
    for k, want in (("loss", lo), ("params", po), ("exp_avg", mo), ("exp_avg_sq", vo)):
        assert _same(got[k], want), (shape, bs, k, _differing(got[k], want))


# ------------------------------------------------------------------ (d) autograd

@pytest.mark.parametrize("name", ("T2", "T5", "T7", "T10"))
def test_forward_tape_and_backward_equal_the_ordered_oracle(dev, name):
    """lbdrn_forward_tape + lbdrn_backward with an upstream gradient that is no MSE gradient, dL/dx asked for."""
    row = BY_NAME[name]
    p0, x, _, dy = inputs(row)
    with O.hidden_activation(row.act):
        y_o, g_o, dx_o = O.backward_ordered(p0.copy(), row.F, row.bc, row.C, row.nl, x, dy)
    p, xd, dyd = (torch.from_numpy(a.copy()).to(dev) for a in (p0, x, dy))
    net = _net(row)
    y, tape = ops.forward_tape(net, p, xd)
    grads, dx = ops.backward(net, p, xd, tape, y, dyd, want_dx=True)
    assert _same(y, y_o), ("y", _differing(y, y_o))
    assert _same(grads, g_o), ("grads", _differing(grads, g_o))
    assert _same(dx, dx_o), ("dx", _differing(dx, dx_o))


# ------------------------------------------------------------------ (e) reproducibility

def _guarded_step(dev, row, fill):
    """lbdrn_train_step through ctypes on the current stream: workspace and outputs filled with `fill` beforehand"""
    p0, x, t, _ = inputs(row)
    net = _net(row)
    A = Arena(dev)
    xd, td = A.const(x, "x"), A.const(t, "t")
    n = p0.size
    p = A.buf(n * 4, 0x00, name="params").write(p0)
    m, v = A.buf(n * 4, 0x00, name="exp_avg"), A.buf(n * 4, 0x00, name="exp_avg_sq")
    loss, grads = A.buf(4, fill, name="loss"), A.buf(n * 4, fill, name="grads")
    g = _lib.Geom(net.C, 1, 1, 1, 0, 1, 1, 1, 0, 0, None, None)      # as ops.train_step sizes it
    nws = _lib.lib().lbdrn_train_workspace(ctypes.byref(g), ctypes.byref(net), row.B)
    ws = A.buf(nws, fill, name="workspace")
    torch.cuda.synchronize(dev)                                      # the fills ran on the default stream
    with torch.cuda.device(dev):
        rc = _lib.lib().lbdrn_train_step(ctypes.byref(net), xd.ptr, td.ptr, row.B, p.ptr, m.ptr, v.ptr, 1, ctypes.c_double(LR),
                                         1, loss.ptr, grads.ptr, ws.ptr, ctypes.c_size_t(nws),
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize(dev)
    assert rc == 0, (rc, (_lib.lib().lbdrn_last_error() or b"").decode())
    A.check()
    return {k: b.numpy(np.float32) for k, b in (("loss", loss), ("grads", grads), ("params", p), ("exp_avg", m),
                                                ("exp_avg_sq", v))}


@pytest.mark.parametrize("name", ("T6", "T8"))
def test_step_bits_do_not_depend_on_the_run_the_stream_or_the_workspace(dev, name):
    """Twice on the current stream and once more on a side stream, each time into a workspace (and outputs) holding 0xFF
    and then 0xA5: the oracle's bits every time."""
    row = BY_NAME[name]
    want = first_step(row)
    side = torch.cuda.Stream(dev)
    for run, stream in (("first", None), ("second", None), ("side stream", side)):
        for fill in (0xFF, 0xA5):
            if stream is None:
                got = _guarded_step(dev, row, fill)
            else:
                with torch.cuda.stream(stream):
                    got = _guarded_step(dev, row, fill)
            _assert_state(got, want, (name, run, hex(fill)))
