"""What tests/test_gpu_thin_rasters.py and tests/test_gpu_dark_tiles.py share on the device: the apply-side comparison of one
row of tests/thin_cases.py with the oracle, one fit of a training row, and its first step against float64.

A plain module: no fixture, no marker; it needs torch and the library, like the tests that import it."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle as O  # noqa: E402
import thin_cases as TC  # noqa: E402
import wide_plan_reference as WR  # noqa: E402
from lbdrn_hip import _lib, ops  # noqa: E402

GEN, MFMA, AUTO = _lib.PATH_GENERIC, _lib.PATH_MFMA, _lib.PATH_AUTO
LOSS_RTOL, M_TOL, V_TOL = 1e-5, 2e-5, 5e-5        # the project's training bounds (tests/test_gpu_train_instances.py)
LR = TC.LR_FIT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def act_id(name):
    return ops.ACT_RELU if name == "relu" else ops.ACT_SINE


@contextlib.contextmanager
def no_ranks():
    """encode.py / decode.py in this process, outside any torchrun launch"""
    saved = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    try:
        yield
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


# ---------------------------------------------------------------------------------------------------------------------
# apply side

def check_features(dev, case, img):
    """lbdrn_features, raster order and gathered, against the oracle: -> (msb, labels, msb_max, device image, device MSB, geometry)"""
    msb, lab, mx = O.split_bits(img, TC.K)
    img_d = ops.to_device_u16(img, dev)
    msb_d, mx_d = ops.split_bits(img_d, TC.K)
    assert mx_d == mx and np.array_equal(ops.from_device_u16(msb_d), msb)
    geom = ops.FeatureGeometry(case.C, case.H, case.W, TC.K, case.D, mx, case.cfg(), dev)
    want = O.features(msb, case.D, case.ocfg(), mx)
    assert np.isfinite(want).all()
    got = ops.features(geom, msb_d).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), case
    idx = np.random.default_rng(case.N).permutation(case.N)[:97].astype(np.int64)
    idx = np.concatenate([idx, idx[:1], [case.N - 1, 0]])
    got = ops.features(geom, msb_d, torch.from_numpy(idx).to(dev)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want[idx])), case
    return msb, lab, mx, img_d, msb_d, geom


def check_networks(dev, case, msb, lab, mx, img_d, msb_d, geom, networks=TC.NETWORKS):
    """decode, evaluation and the fast passes of every network against the oracle: -> {network: worst fast / canonical - 1}"""
    worst = {}
    for bc, nl, act in networks:
        rng = np.random.default_rng([case.C, case.H, case.W, case.D, bc, nl])
        params = TC.rand_params(rng, case.F, bc, case.C, nl, gain=2.0)
        with O.hidden_activation(act):
            out_o, y_o = O.decode(msb, TC.K, case.D, case.ocfg(), params, bc, nl, mx, want_y=True)
            sse_o = O.eval_sse(msb, lab, case.D, case.ocfg(), params, bc, nl, mx)
        assert np.isfinite(y_o).all() and np.isfinite(sse_o) and sse_o > 0
        net = ops.make_net(case.F, bc, case.C, nl, act_id(act))
        p_d = torch.from_numpy(params).to(dev)
        tag = (case, bc, nl, act)
        fused = TC.fused_apply_takes(case.C, case.D, case.P, case.F, bc, nl, act)
        for path in (GEN, MFMA if fused else AUTO):
            out, y = ops.decode_fused(geom, net, msb_d, p_d, want_y=True, path=path)
            assert np.array_equal(bits(y.cpu().numpy()), bits(y_o)), (tag, path)
            assert np.array_equal(ops.from_device_u16(out), out_o), (tag, path)
            sse = float(ops.eval_sse(geom, net, img_d, msb_d, p_d, path=path).item())
            assert abs(sse - sse_o) <= 1e-11 * max(1.0, abs(sse_o)), (tag, path, sse, sse_o)
        if not fused:                          # the plan does not fit this network, on any raster: refused, never a quiet fall-back
            for call in (lambda: ops.decode_fused(geom, net, msb_d, p_d, path=MFMA), lambda: ops.eval_sse(geom, net, img_d, msb_d, p_d, path=MFMA)):
                with pytest.raises(_lib.LbdrnError) as e:
                    call()
                assert e.value.code == _lib.E_UNSUPPORTED, tag
        canon = float(ops.eval_sse(geom, net, img_d, msb_d, p_d).item())
        for x16 in (False, True):
            fast = [float(ops.eval_sse(geom, net, img_d, msb_d, p_d, fast=True, x16=x16, background=b).item()) for b in (False, False, True)]
            assert fast[0] == fast[1] == fast[2], (tag, x16, fast)
            rel = abs(fast[0] - canon) / canon
            worst[(bc, nl, act)] = max(worst.get((bc, nl, act), 0.0), rel)
            assert rel <= 1e-6, (tag, x16, fast[0], canon)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# training side

class Fit:
    """One fit of a training row on the device, prepared for minibatches of bs rows on one path."""

    def __init__(self, dev, row, bs, path, inputs=None):
        self.row, self.bs, self.dev, self.path = row, bs, dev, path
        self.img, self.p0, self.perm_np = inputs or TC.train_inputs(row)
        self.msb, self.lab, self.mx = O.split_bits(self.img, TC.K)
        self.img_d, self.msb_d = ops.to_device_u16(self.img, dev), ops.to_device_u16(self.msb, dev)
        self.geom = ops.FeatureGeometry(row.C, row.H, row.W, TC.K, row.D, self.mx, row.case.cfg(row.act), dev)
        self.net = ops.make_net(row.F, row.bc, row.C, row.nl, act_id(row.act))
        self.perm = torch.from_numpy(self.perm_np).to(dev)
        self.ws = ops.TrainWorkspace(self.geom, self.net, bs, dev).prepare(self.img_d, self.msb_d, path)

    def epochs(self, alone, epochs, perm=None, lr=LR):
        """`epochs` lbdrn_train_epoch calls from the initial state -> [params, exp_avg, exp_avg_sq, losses]"""
        perm = self.perm if perm is None else perm
        steps = (perm.numel() + self.bs - 1) // self.bs
        p = torch.from_numpy(self.p0.copy()).to(self.dev)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        losses = torch.zeros(steps, dtype=torch.float32, device=self.dev)
        for e in range(epochs):
            ops.train_epoch(self.geom, self.net, self.img_d, self.msb_d, perm, self.bs, p, m, v, e * steps, lr, losses, self.path,
                            self.ws, alone=alone)
        return [t.cpu().numpy() for t in (p, m, v, losses)]


def check_instance(row, fit):
    """What the library tells of the plan it made for this row ON THIS RASTER (it has no call that names a kernel): the
    features the fused step multiplies, how many fits it steps per launch -- 4 on k_train_stream / k_train_split, 1 on the tile
    kernel and at bc >= 128 --, that PATH_MFMA is not refused, and at bc >= 128 the workspace size of the restated wide plan.
    Which template instance that plan steps a minibatch of B rows on is the restatement's part
    (tests/test_thin_rasters_host.py::test_training_rows_step_on_the_kernels_they_name, at the very B the tests use)."""
    assert ops.train_step_features(fit.geom, fit.net) == row.Fe
    assert ops.train_group_size(row.C, row.H, row.W, TC.K, row.D, row.case.cfg(row.act), row.bc, row.nl) == row.group_size()
    if row.bc != 64:
        assert fit.ws.nbytes == WR.workspace_bytes(row.shape(), row.bc, row.H, row.W, fit.bs)


def centre_columns(row):
    """flat indices of W_0[n][centre of band c]: the columns a step with Fe = F - C leaves out"""
    side = 2 * row.D + 1
    centre = 2 * row.case.P + np.arange(row.C) * side * side + row.D * side + row.D
    return (np.arange(row.bc)[:, None] * row.F + centre[None, :]).ravel()


def rel_distance(got, want):
    top = np.abs(want).max()
    d = np.abs(got - want).max()
    return float(d / top) if top > 0 else (0.0 if d == 0 else np.inf)


def first_step_against_float64(dev, row, inputs=None, label=None, B=TC.BS_FIRST):
    """The first step of PATH_GENERIC and PATH_MFMA from a zero state against tests/train_step_f64.py, under the rule of
    tests/test_gpu_train_instances.py::test_first_step_against_float64.  -> {path: (loss, exp_avg, exp_avg_sq) distances}"""
    img, p0, perm = inputs or TC.train_inputs(row)
    x, t, b, loss64, g64 = TC.first_step_f64(row, img, p0, perm, B)
    m64, v64 = 0.1 * g64, 0.001 * g64 * g64
    dist = {}
    for path in (GEN, MFMA):
        fit = Fit(dev, row, B, path, (img, p0, perm))
        if path == MFMA:
            check_instance(row, fit)
        p, m, v, losses = fit.epochs(alone=row.alone and path == MFMA, epochs=1, perm=fit.perm[:B].contiguous())
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(losses).all(), (row, path)
        dist[path] = (abs(float(losses[0]) - loss64) / loss64, rel_distance(m, m64), rel_distance(v, v64))
        if row.Fe == row.F - row.C:
            cols = centre_columns(row)
            assert np.array_equal(bits(p[cols]), bits(p0[cols])), path
            assert not m[cols].any() and not v[cols].any(), path
            assert not g64[cols].any()
        assert np.abs(p - p0).max() > 0
    print(f"\n{label or row.id}: distance from float64 (loss, exp_avg, exp_avg_sq) generic %.2e %.2e %.2e | fused %.2e %.2e %.2e"
          % (dist[GEN] + dist[MFMA]))
    for name, bound, dg, df in zip(("loss", "exp_avg", "exp_avg_sq"), (LOSS_RTOL, M_TOL, V_TOL), dist[GEN], dist[MFMA]):
        assert dg <= bound, (name, "generic", dg)
        assert df <= max(bound, 2 * dg), (name, "fused", df, dg)
    return dist
