"""Every template instance of the fused bc = 64 training step, stepped once on the device: alone and in groups.

The table is the census of tests/train_plan_reference.py (every reachable k_train_stream / k_train_split / tile-kernel
instance at its smallest real shape, plus the class boundaries of Fe and a full and a part-filled last strip per LQ);
tests/test_train_plan_host.py proves on the CPU that the table is complete and that each row selects the instance it is
named after.  Per row, on a 13 x 11 raster (minibatches of 100 rows = two workgroups, the second part-filled, then 43
rows = less than one; one variant per kernel family with 71 + 71 + 1 rows):

  (a) the first step from a zero state -- loss, exp_avg = 0.1 g, exp_avg_sq = 0.001 g^2 -- of PATH_MFMA and of PATH_GENERIC
      against the float64 step of tests/train_step_f64.py, at the project's bounds (loss 1e-5 relative, exp_avg 2e-5 and
      exp_avg_sq 5e-5 of the largest entry); the fused step may pass a bound only up to twice the generic step's own
      distance from float64 in the same quantity;
  (b) the window-centre columns of W_0 and their moments bit-unchanged wherever the step skips them;
  (c) two epochs bit-identical run to run and with and without the LBDRN_TRAIN_ALONE hint;
  (d) groups of 2, 3 and 4 fits -- own image, largest MSB value, parameters and permutation each -- bit-identical, fit by
      fit, to the single calls; per kernel family also in reversed order and with `losses` NULL for fits 0 and 2;
  (e) refusals that write nothing (guarded state buffers, tests/guarded.py);
  (f) the instance the restatement names for the row, and what the library tells of it, asserted per test.

What a wrong kernel would trip: a wrong strip bound in the loop schedule (NT0C = 0) drops or doubles columns of dW_0 --
(a) of stream-LQ48-nl2-loop-sine-Fe130 (nine strips, the last holding two features) and stream-LQ64-nl2-loop-sine-Fe216;
a wrong fit index in k_reduce_adam gives fit k > 0 the state of another fit -- (d) of every streamed row, whose fits differ
in every input; perm[0] in perm_next reaching a grouped kernel would feed fit k rows of fit 0 -- (d) likewise, and the
reversed-order variant where fit 0 is another fit."""
import ctypes
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
import train_plan_reference as R  # noqa: E402
from guarded import Arena  # noqa: E402
from lbdrn_hip import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
GEN, MFMA = _lib.PATH_GENERIC, _lib.PATH_MFMA
LOSS_RTOL, M_TOL, V_TOL = 1e-5, 2e-5, 5e-5        # the project's training bounds (tests/test_gpu_fuzz.py)
LR = 1e-3

ROWS = R.census()[0]


def _family_rows():
    """one row per kernel family (Sine, two hidden layers where the family has them): the variants that are run once"""
    out = {}
    for r in ROWS:
        if r.shape.act == "sine" and r.shape.nl >= 2 and r.Fe > 16:
            out.setdefault(r.family, r)
    return out


FAMILY = _family_rows()
CASES = [pytest.param(r, R.BS, id=r.id) for r in ROWS] + [pytest.param(r, R.BS_TAIL, id=r.id + "-tail1") for r in FAMILY.values()]


def _bits(a):
    return a.view(np.int32)


class Fit:
    """One fit of a row on the device: its own image, largest MSB value, parameters, permutation and prepared workspace."""

    def __init__(self, dev, shape, seed, k, bs, path=MFMA):
        self.shape, self.bs, self.dev = shape, bs, dev
        self.img, self.p0, self.perm_np = R.fit_inputs(shape, seed, k)
        self.msb, self.lab, self.mx = O.split_bits(self.img, R.K)
        self.img_d, self.msb_d = ops.to_device_u16(self.img, dev), ops.to_device_u16(self.msb, dev)
        self.geom = ops.FeatureGeometry(shape.C, R.H, R.W, R.K, shape.D, self.mx, shape.featcfg(), dev)
        self.net = ops.make_net(shape.F, 64, shape.C, shape.nl, 1 if shape.act == "relu" else 0)
        self.perm = torch.from_numpy(self.perm_np).to(dev)
        self.path = path
        self.ws = ops.TrainWorkspace(self.geom, self.net, bs, dev).prepare(self.img_d, self.msb_d, path)
        self.steps = (len(self.perm_np) + bs - 1) // bs

    def state(self):
        p = torch.from_numpy(self.p0.copy()).to(self.dev)
        return p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(self.steps, dtype=torch.float32, device=self.dev)

    def epochs(self, alone, epochs=2, perm=None):
        """`epochs` single lbdrn_train_epoch calls from the initial state -> [params, exp_avg, exp_avg_sq, losses]"""
        p, m, v, losses = self.state()
        perm = self.perm if perm is None else perm
        steps = (perm.numel() + self.bs - 1) // self.bs
        for e in range(epochs):
            ops.train_epoch(self.geom, self.net, self.img_d, self.msb_d, perm, self.bs, p, m, v, e * steps, LR, losses,
                            self.path, self.ws, alone=alone)
        return [t.cpu().numpy() for t in (p, m, v, losses)]


def _group_epochs(fits, order, no_losses=()):
    """two lbdrn_train_epoch_group calls over fits[k] for k in order -> {k: [params, exp_avg, exp_avg_sq, losses]}"""
    sel = [fits[k] for k in order]
    st = [f.state() for f in sel]
    losses = [None if j in no_losses else s[3] for j, s in enumerate(st)]
    for e in range(2):
        ops.train_epoch_group([f.geom for f in sel], sel[0].net, [f.img_d for f in sel], [f.msb_d for f in sel],
                              [f.perm for f in sel], sel[0].bs, [s[0] for s in st], [s[1] for s in st], [s[2] for s in st],
                              e * sel[0].steps, LR, losses, MFMA, [f.ws for f in sel])
    return {k: [t.cpu().numpy() for t in s] for k, s in zip(order, st)}


def _centre_columns(shape):
    """flat indices of W_0[n][centre of band c]: the columns a step with Fe = F - C leaves out"""
    side = 2 * shape.D + 1
    centre = 2 * shape.P + np.arange(shape.C) * side * side + shape.D * side + shape.D
    return (np.arange(64)[:, None] * shape.F + centre[None, :]).ravel()


def _check_instance(row, fit):
    """(f): the row steps on the instance it is named after, as far as the restatement and the library tell"""
    s = row.shape
    assert R.instance_id(s.instance(alone=row.alone, count=1, B=R.BS), row.Fe) == row.id
    assert ops.train_step_features(fit.geom, fit.net) == row.Fe
    assert (row.Fe == s.F - s.C) == (s.colors and s.relative and s.D > 0 and row.inst[0] != "tile")
    gs = ops.train_group_size(s.C, R.H, R.W, R.K, s.D, s.featcfg(), 64, s.nl)
    assert gs == (R.MAX_GROUP if row.inst[0] != "tile" else 1) == (ops.train_group_max() if R.takes_groups(s.plan()) else 1)
    if row.inst[0] == "split" and row.LQ != R.SPLIT_WIDE_LQ:     # the one-row minibatch of a lone fit goes out on k_train_stream
        assert s.instance(alone=True, count=1, B=1) == ("stream", row.LQ, 2, row.NT0, s.act)
        assert s.instance(alone=False, count=1, B=2)[0] == "stream"


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_first_step_against_float64(dev, row):
    """(a), (b), (f).  Distances from float64 are printed before they are asserted."""
    s = row.shape
    seed = R.row_seed(row.id)
    x, t, p0, b, loss64, g64 = R.first_step_f64(s, seed)
    m64, v64 = 0.1 * g64, 0.001 * g64 * g64
    dist = {}
    for path in (GEN, MFMA):
        fit = Fit(dev, s, seed, 0, R.BS, path)
        assert np.array_equal(fit.p0, p0) and np.array_equal(fit.perm_np[:R.BS], b)
        if path == MFMA:
            _check_instance(row, fit)
        p, m, v, losses = fit.epochs(alone=row.alone and path == MFMA, epochs=1, perm=fit.perm[:R.BS].contiguous())
        dist[path] = (abs(float(losses[0]) - loss64) / loss64, np.abs(m - m64).max() / np.abs(m64).max(),
                      np.abs(v - v64).max() / np.abs(v64).max())
        if row.Fe == s.F - s.C:                                          # (b)
            cols = _centre_columns(s)
            assert np.array_equal(_bits(p[cols]), _bits(p0[cols])), path
            assert not m[cols].any() and not v[cols].any(), path
            assert not g64[cols].any()
        assert np.abs(p - p0).max() > 0 and np.isfinite(p).all()
    print(f"\n{row.id}: distance from float64 (loss, exp_avg, exp_avg_sq) generic %.2e %.2e %.2e | fused %.2e %.2e %.2e"
          % (dist[GEN] + dist[MFMA]))
    for name, bound, dg, df in zip(("loss", "exp_avg", "exp_avg_sq"), (LOSS_RTOL, M_TOL, V_TOL), dist[GEN], dist[MFMA]):
        assert dg <= bound, (name, "generic", dg)
        assert df <= max(bound, 2 * dg), (name, "fused", df, dg)


@pytest.mark.parametrize("row,bs", CASES)
def test_epochs_and_groups_are_bit_identical(dev, row, bs):
    """(b), (c), (d), (f)."""
    s = row.shape
    seed = R.row_seed(row.id)
    grouped = row.inst[0] != "tile"
    fits = [Fit(dev, s, seed, k, bs) for k in range(R.MAX_GROUP if grouped else 1)]
    assert len({f.mx for f in fits}) == len(fits) and fits[0].steps == (3 if bs == R.BS_TAIL else 2)
    _check_instance(row, fits[0])
    # (c) run to run, and the hint of a lone fit (k_train_split where the shape has it) changes no bit
    single = {k: f.epochs(alone=row.alone) for k, f in enumerate(fits)}
    for alone in (row.alone, not row.alone):
        again = fits[0].epochs(alone=alone)
        assert all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(single[0], again)), alone
    p, m, v, losses = single[0]
    assert np.isfinite(p).all() and np.isfinite(losses).all() and np.abs(m).max() > 0
    if row.Fe == s.F - s.C:                                              # (b) after two epochs
        cols = _centre_columns(s)
        assert np.array_equal(_bits(p[cols]), _bits(fits[0].p0[cols])) and not m[cols].any() and not v[cols].any()
    # every step of the epochs -- the part-filled workgroup, the short minibatch, the one-row tail -- trains as the generic
    # kernels do (tests/test_gpu_fuzz.py's bound on the losses of a few steps)
    gen = Fit(dev, s, seed, 0, bs, GEN).epochs(alone=False)
    np.testing.assert_allclose(losses, gen[3], rtol=5e-5)
    if not grouped:
        return
    # (d) groups against the single calls
    runs = [tuple(range(n)) for n in (2, 3, 4)]
    variants = []
    if FAMILY.get(row.family) is row:
        runs.append((3, 2, 1, 0))
        variants.append(((0, 1, 2, 3), (0, 2)))
    for order in runs:
        got = _group_epochs(fits, order)
        for k in order:
            for name, a, c in zip(("params", "exp_avg", "exp_avg_sq", "losses"), got[k], single[k]):
                assert np.array_equal(_bits(a), _bits(c)), (order, k, name)
    for order, no_losses in variants:
        got = _group_epochs(fits, order, no_losses)
        for j, k in enumerate(order):
            for name, a, c in list(zip(("params", "exp_avg", "exp_avg_sq", "losses"), got[k], single[k]))[:3 if j in no_losses else 4]:
                assert np.array_equal(_bits(a), _bits(c)), (order, no_losses, k, name)
            if j in no_losses:
                assert not got[k][3].any()                               # (its zeroed array was not handed over: untouched)


def _raw_group(count, slots, net, n, bs, path, ref):
    """lbdrn_train_epoch_group with `count` as given over the pointer arrays of `slots` (dicts of guarded buffers)"""
    arr = lambda key: (ctypes.c_void_p * len(slots))(*[s[key].ptr if hasattr(s[key], "ptr") else ctypes.c_void_p(s[key].data_ptr()) for s in slots])
    garr = (ctypes.POINTER(_lib.Geom) * len(slots))(*[ctypes.pointer(s["geom"].c) for s in slots])
    ops._call(_lib.lib().lbdrn_train_epoch_group, ref, count, ctypes.cast(garr, ctypes.c_void_p), ctypes.byref(net), arr("img"),
              arr("msb"), arr("perm"), n, bs, arr("p"), arr("m"), arr("v"), 0, LR, arr("losses"), arr("ws"), slots[0]["ws"].nbytes, path)


def test_refusals_write_nothing(dev):
    """(e).  A group of 0 or of 5 fits is refused (LBDRN_E_ARG: 1 .. lbdrn_train_group_max()); a group of two of a shape
    without a fused step -- three hidden ReLU layers -- answers LBDRN_E_UNSUPPORTED under LBDRN_PATH_MFMA.  No byte of the
    parameters, moments or losses changes and no guard is touched.  (A shape whose fused step takes one fit per launch --
    the nl = 3 tile kernel -- is not refused: include/lbdrn_hip.h has its fits run one after another, and they must end on
    the bits of the single calls.)"""
    seed = 0
    streamed = R.Shape(0, 0, 1, 1, 4, 2, 2, "sine")
    nofused = R.Shape(0, 0, 1, 1, 4, 2, 3, "relu")
    tile = R.Shape(0, 0, 1, 1, 3, 1, 3, "sine")
    assert R.takes_groups(streamed.plan()) and nofused.plan() is None and tile.plan()["kind"] == "tile"
    n = R.H * R.W
    for shape, count, nslots, path, code in ((streamed, 0, 4, MFMA, _lib.E_ARG), (streamed, 5, 5, MFMA, _lib.E_ARG),
                                             (nofused, 2, 2, MFMA, _lib.E_UNSUPPORTED)):
        arena = Arena(dev)
        rng = np.random.default_rng(count)
        slots = []
        net = ops.make_net(shape.F, 64, shape.C, shape.nl, 1 if shape.act == "relu" else 0)
        for k in range(nslots):
            img, p0, perm = R.fit_inputs(shape, seed, k % 4)
            msb, _, mx = O.split_bits(img, R.K)
            geom = ops.FeatureGeometry(shape.C, R.H, R.W, R.K, shape.D, mx, shape.featcfg(), dev)
            nbytes = _lib.lib().lbdrn_train_workspace(ctypes.byref(geom.c), ctypes.byref(net), R.BS)
            assert nbytes > 0
            slots.append(dict(geom=geom, img=arena.const(img), msb=arena.const(msb), perm=arena.const(perm), p=arena.const(p0),
                              m=arena.const(rng.standard_normal(len(p0)).astype(np.float32)),
                              v=arena.const(rng.random(len(p0)).astype(np.float32)),
                              losses=arena.const(np.full(2, 7.0, np.float32)), ws=arena.buf(nbytes, 0xA5)))
        with pytest.raises(_lib.LbdrnError) as e:
            _raw_group(count, slots, net, n, R.BS, path, slots[0]["p"].t)
        assert e.value.code == code, (count, e.value)
        torch.cuda.synchronize(dev)
        arena.check()
        for s in slots:
            assert bool((s["ws"].as_u8() == 0xA5).all())                 # the workspaces were not touched either
    # the tile kernel's shape: a group of two runs fit after fit, same bits
    fits = [Fit(dev, tile, seed, k, R.BS) for k in range(2)]
    assert ops.train_group_size(tile.C, R.H, R.W, R.K, tile.D, tile.featcfg(), 64, 3) == 1
    single = [f.epochs(alone=False) for f in fits]
    got = _group_epochs(fits, (0, 1))
    for k in range(2):
        assert all(np.array_equal(_bits(a), _bits(c)) for a, c in zip(got[k], single[k])), k
