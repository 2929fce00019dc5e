"""Every template instance of the bc = 128 / 256 training step (k_train_half<LQ, NL, NT> -> k_dw_wide<NT, NL> -> k_reduce_adam,
csrc/train_wide.inc), stepped on the device against a float64 step -- every step of an epoch, not only the first.

The table is the census of tests/wide_plan_reference.py: the 20 k_train_half instances (and with them the 4 of k_dw_wide) at
their smallest real shapes, then at bc = 256, nl = 2 the class boundaries of Fe, the two shapes the row pitch pushes to LQ 64,
Fe = 252, a full and a part-filled last strip per LQ and every residue of NT0 mod 4.  tests/test_wide_plan_host.py proves on
the CPU that the table is complete and that the minibatches below have the geometry named here.

The comparison tool is an epoch at lr = 0.0 from zero moments.  The parameters then never move (asserted first, bit for bit,
on both paths), every step's gradient is taken at p0, and after S steps
    exp_avg = sum_s 0.1 0.9^(S-1-s) g_s,   exp_avg_sq = sum_s 0.001 0.999^(S-1-s) g_s^2,   losses[s] = loss_s
-- all three computed in float64 (tests/train_step_f64.py) on the oracle's features and labels.  A step's loss is formed before
its weight gradient, so only the moments see a wrong k_dw_wide product or a stale row of an earlier, larger minibatch left in
the operands of k_dw_wide; after the last step such a row still carries a tenth of its weight.

Per census row, on the 13 x 11 raster, PATH_GENERIC and PATH_MFMA, two permutations of the 143 pixels:
    bs = 90:  steps of 90 and 53 rows -- three workgroups (an odd count: the zero-filled half block, and a part-filled last
              workgroup), then two;
    bs = 128: steps of 128 and 15 rows -- one workgroup after four: rows 32..63 hold the first step's dz unless zeroed.
  (a) losses within 1e-5 relative of float64, exp_avg / exp_avg_sq within the project's 2e-5 / 5e-5 of the largest entry, on both
      paths; the fused step may pass a bound only up to twice the generic step's own distance from float64 in that quantity;
      the same per parameter block (W_0, b_0, W_1, b_1, W_last, b_last, each relative to the block's largest float64 entry):
      fused <= max(project bound, 2 x the generic step's distance in that block) -- a dropped or doubled 16-column strip of
      dW_0 is small against the head's gradient, not against W_0's own.  Every distance is printed before it is asserted;
  (b) where Fe = F - C the window-centre columns of W_0 stay bit-unchanged and their moments exact zeros;
  (c) lbdrn_train_step_features = Fe, and the restated workspace size is the library's;
  (d) at lr = 1e-3 two epochs are bit-identical run to run, and PATH_AUTO gives the bits of PATH_MFMA.
Per family (bc, nl) at the headline features (8 bands, D = 2, relative colours: Fe 192, LQ 48, NT0 12), same comparison:
  bs = 71 (71, 71, 1: a one-row tail); on a 96 x 97 raster bs = 1040 (33 workgroups, two slices, the second of 64 rows so
  that three of its waves have none; a short step after eight long ones) and bs = 9312 (291 workgroups, 10 slices: XCDs 0 and
  1 walk two slices each); groups of 2, 3 and 4 fits bit-identical to the single calls; refusals that write nothing.

What a wrong kernel would trip: the zero-fill of the half block skipped -- exp_avg of the bs = 128 rows (their losses pass);
`4 * im + vt < NT0` off by one in k_dw_wide -- W_0's block of the rows whose NT0 is no multiple of four."""
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
import wide_plan_reference as WR  # noqa: E402
from guarded import Arena  # noqa: E402
from lbdrn_hip import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
GEN, MFMA, AUTO = _lib.PATH_GENERIC, _lib.PATH_MFMA, _lib.PATH_AUTO
LOSS_RTOL, M_TOL, V_TOL = 1e-5, 2e-5, 5e-5        # the project's training bounds (tests/test_gpu_fuzz.py)
LR = 1e-3

ROWS = WR.census()[0]
FAMILIES = [(bc, nl) for bc in WR.BCS for nl in WR.NLS]


def _bits(a):
    return a.view(np.int32)


class Fit:
    """One fit of a shape at a width on the device: its own image, largest MSB value, parameters, permutation and prepared
    workspace."""

    def __init__(self, dev, shape, bc, k, bs, path, h=WR.H, w=WR.W, seed=0):
        self.shape, self.bc, self.bs, self.dev, self.path, self.h, self.w = shape, bc, bs, dev, path, h, w
        self.img, self.p0, self.perm_np = WR.fit_inputs(shape, bc, seed, k, h, w)
        self.msb, self.lab, self.mx = O.split_bits(self.img, WR.K)
        self.img_d, self.msb_d = ops.to_device_u16(self.img, dev), ops.to_device_u16(self.msb, dev)
        self.geom = ops.FeatureGeometry(shape.C, h, w, WR.K, shape.D, self.mx, shape.featcfg(), dev)
        self.net = ops.make_net(shape.F, bc, shape.C, shape.nl, 0)
        self.perm = torch.from_numpy(self.perm_np).to(dev)
        self.ws = ops.TrainWorkspace(self.geom, self.net, bs, dev).prepare(self.img_d, self.msb_d, path)
        self.steps = (len(self.perm_np) + bs - 1) // bs

    def state(self):
        p = torch.from_numpy(self.p0.copy()).to(self.dev)
        return p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(self.steps, dtype=torch.float32, device=self.dev)

    def epochs(self, lr, epochs):
        """`epochs` lbdrn_train_epoch calls from the initial state -> [params, exp_avg, exp_avg_sq, losses]"""
        p, m, v, losses = self.state()
        for e in range(epochs):
            ops.train_epoch(self.geom, self.net, self.img_d, self.msb_d, self.perm, self.bs, p, m, v, e * self.steps, lr, losses,
                            self.path, self.ws)
        return [t.cpu().numpy() for t in (p, m, v, losses)]


def _centre_columns(shape, bc):
    """flat indices of W_0[n][centre of band c]: the columns a step with Fe = F - C leaves out"""
    side = 2 * shape.D + 1
    centre = 2 * shape.P + np.arange(shape.C) * side * side + shape.D * side + shape.D
    return (np.arange(bc)[:, None] * shape.F + centre[None, :]).ravel()


def _rel(got, want):
    """largest difference relative to the largest float64 entry (a block of exact zeros admits exact zeros only)"""
    top = np.abs(want).max()
    d = np.abs(got - want).max()
    return float(d / top) if top > 0 else (0.0 if d == 0 else np.inf)


def _against_float64(dev, shape, bc, bs, h=WR.H, w=WR.W, label="", generic_at_project_bound=True):
    """The lr = 0 epoch of fit 0 on both paths against float64: bit-unchanged parameters, (a) whole and per block, (b)."""
    img, p0, perm = WR.fit_inputs(shape, bc, 0, 0, h, w)
    x, t = WR.features_and_labels_f64(shape, img)
    loss64, m64, v64, grads = WR.zero_lr_epoch_f64(shape, bc, x, t, p0, perm, bs)          # once, for both paths
    assert len(grads) == (h * w + bs - 1) // bs and all(np.abs(g).max() > 0 for g in grads)
    blocks = WR.blocks(shape, bc)
    dist = {}
    for path in (GEN, MFMA):
        fit = Fit(dev, shape, bc, 0, bs, path, h, w)
        assert np.array_equal(fit.p0, p0) and np.array_equal(fit.perm_np, perm)
        p, m, v, losses = fit.epochs(0.0, 1)
        assert np.array_equal(_bits(p), _bits(p0)), (label, path, "a zero step size moved the parameters")
        assert np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(losses).all(), (label, path)
        d = {"loss": float((np.abs(losses.astype(np.float64) - loss64) / loss64).max()),
             "exp_avg": _rel(m, m64), "exp_avg_sq": _rel(v, v64)}
        for name, sl in blocks:
            d["exp_avg/" + name] = _rel(m[sl], m64[sl])
            d["exp_avg_sq/" + name] = _rel(v[sl], v64[sl])
        dist[path] = d
        if shape.Fe == shape.F - shape.C:                                    # (b)
            cols = _centre_columns(shape, bc)
            assert not m[cols].any() and not v[cols].any(), (label, path)
            assert not m64[cols].any()
    g, f = dist[GEN], dist[MFMA]
    print(f"\n{label} bs={bs} ({len(grads)} steps): distance from float64, generic | fused")
    print("  whole  loss %.2e | %.2e   exp_avg %.2e | %.2e   exp_avg_sq %.2e | %.2e"
          % (g["loss"], f["loss"], g["exp_avg"], f["exp_avg"], g["exp_avg_sq"], f["exp_avg_sq"]))
    for name, _ in blocks:
        print("  %-6s exp_avg %.2e | %.2e   exp_avg_sq %.2e | %.2e"
              % (name, g["exp_avg/" + name], f["exp_avg/" + name], g["exp_avg_sq/" + name], f["exp_avg_sq/" + name]))
    for key in g:
        bound = LOSS_RTOL if key == "loss" else V_TOL if key.startswith("exp_avg_sq") else M_TOL
        if key == "loss" or (generic_at_project_bound and "/" not in key):
            assert g[key] <= bound, (label, bs, key, "generic", g[key])
        assert f[key] <= max(bound, 2 * g[key]), (label, bs, key, "fused", f[key], "generic", g[key])


@pytest.mark.parametrize("bs", (WR.BS_ODD, WR.BS_STALE), ids=("bs90", "bs128"))
@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_every_step_against_float64(dev, row, bs):
    """(a), (b), (c) of a census row at one of its two permutations."""
    s = row.shape
    fit = Fit(dev, s, row.bc, 0, bs, MFMA)                                  # (c)
    assert ops.train_step_features(fit.geom, fit.net) == row.Fe == WR.plan(s, row.bc)["Fe"]
    assert (row.Fe == s.F - s.C) == (s.colors and s.relative and s.D > 0)
    assert fit.ws.nbytes == WR.workspace_bytes(s, row.bc, WR.H, WR.W, bs)
    assert ops.train_group_size(s.C, WR.H, WR.W, WR.K, s.D, s.featcfg(), row.bc, s.nl) == 1
    _against_float64(dev, s, row.bc, bs, label=row.id)


@pytest.mark.parametrize("row", [pytest.param(r, id=r.id) for r in ROWS])
def test_epochs_are_bit_identical_and_auto_is_the_fused_step(dev, row):
    """(d), and (b) after two epochs of real updates."""
    s = row.shape
    first = Fit(dev, s, row.bc, 0, WR.BS_ODD, MFMA).epochs(LR, 2)
    again = Fit(dev, s, row.bc, 0, WR.BS_ODD, MFMA).epochs(LR, 2)
    auto = Fit(dev, s, row.bc, 0, WR.BS_ODD, AUTO).epochs(LR, 2)
    for name, a, b, c in zip(("params", "exp_avg", "exp_avg_sq", "losses"), first, again, auto):
        assert np.array_equal(_bits(a), _bits(b)), ("run to run", name)
        assert np.array_equal(_bits(a), _bits(c)), ("PATH_AUTO", name)
    p, m, v, losses = first
    p0 = WR.fit_inputs(s, row.bc, 0, 0)[1]
    assert np.isfinite(p).all() and np.isfinite(losses).all() and np.abs(p - p0).max() > 0
    if row.Fe == s.F - s.C:
        cols = _centre_columns(s, row.bc)
        assert np.array_equal(_bits(p[cols]), _bits(p0[cols])) and not m[cols].any() and not v[cols].any()


@pytest.mark.parametrize("case", ("tail71", "big1040", "big9312"))
@pytest.mark.parametrize("bc,nl", FAMILIES, ids=[f"bc{bc}-nl{nl}" for bc, nl in FAMILIES])
def test_families_at_the_headline_features(dev, bc, nl, case):
    """The headline features at every width and depth: a one-row tail, more than one slice with idle waves, more than eight
    slices.  On the large raster the float32 sums of both paths are looser than on the small one: the generic step's moments
    are printed, the fused step's are held to max(project bound, 2 x the generic step's distance), whole and per block."""
    s = R.Shape(*WR.HEADLINE, nl, "sine")
    p = WR.plan(s, bc)
    assert (p["Fe"], p["LQ"], p["NT0"]) == (192, 48, 12)
    label = f"headline-bc{bc}-nl{nl}-{case}"
    if case == "tail71":
        _against_float64(dev, s, bc, WR.BS_TAIL, label=label)
    else:
        bs = 1040 if case == "big1040" else WR.BIG_H * WR.BIG_W
        g = WR.launches(s, bc, bs)
        assert g["zero_fill"] and (g["nslices"], g["idle_waves"]) == ((2, 3) if bs == 1040 else (10, 3))
        _against_float64(dev, s, bc, bs, WR.BIG_H, WR.BIG_W, label=label, generic_at_project_bound=False)


def _group_epochs(fits, order, no_losses=()):
    """two lbdrn_train_epoch_group calls over fits[k] for k in order -> {k: [params, exp_avg, exp_avg_sq, losses]}"""
    sel = [fits[k] for k in order]
    st = [f.state() for f in sel]
    for j in no_losses:
        st[j][3].fill_(7.0)
    losses = [None if j in no_losses else s[3] for j, s in enumerate(st)]
    for e in range(2):
        ops.train_epoch_group([f.geom for f in sel], sel[0].net, [f.img_d for f in sel], [f.msb_d for f in sel],
                              [f.perm for f in sel], sel[0].bs, [s[0] for s in st], [s[1] for s in st], [s[2] for s in st],
                              e * sel[0].steps, LR, losses, MFMA, [f.ws for f in sel])
    return {k: [t.cpu().numpy() for t in s] for k, s in zip(order, st)}


@pytest.mark.parametrize("bc,nl", FAMILIES, ids=[f"bc{bc}-nl{nl}" for bc, nl in FAMILIES])
def test_groups_run_fit_after_fit_on_the_same_bits(dev, bc, nl):
    """lbdrn_train_epoch_group with 2, 3 and 4 fits of a wide shape under PATH_MFMA: the step takes one fit per launch, the fits
    run one after another (include/lbdrn_hip.h) and end on the bits of the single calls; `losses` NULL for one fit leaves its
    array alone.  The fits differ in image, largest MSB value, parameters and permutation."""
    s = R.Shape(*WR.HEADLINE, nl, "sine")
    fits = [Fit(dev, s, bc, k, WR.BS_ODD, MFMA) for k in range(4)]
    assert len({f.mx for f in fits}) == 4 and fits[0].steps == 2
    assert all(not np.array_equal(fits[0].perm_np, f.perm_np) and not np.array_equal(fits[0].p0, f.p0) for f in fits[1:])
    single = {k: f.epochs(LR, 2) for k, f in enumerate(fits)}
    for order, no_losses in (((0, 1), ()), ((0, 1, 2), ()), ((0, 1, 2, 3), ()), ((3, 1, 0), (1,))):
        got = _group_epochs(fits, order, no_losses)
        for j, k in enumerate(order):
            for name, a, c in list(zip(("params", "exp_avg", "exp_avg_sq", "losses"), got[k], single[k]))[:3 if j in no_losses else 4]:
                assert np.array_equal(_bits(a), _bits(c)), (order, no_losses, k, name)
            if j in no_losses:
                assert (got[k][3] == 7.0).all()                              # (not handed over: untouched)


@pytest.mark.parametrize("act,nl,bc", (("relu", 2, 128), ("sine", 3, 256)), ids=("relu-bc128", "nl3-bc256"))
def test_refusals_write_nothing(dev, act, nl, bc):
    """ReLU at bc = 128 and three hidden layers at bc = 256 have no fused step: lbdrn_train_prepare, lbdrn_train_epoch and
    lbdrn_train_epoch_group (one fit and two) under PATH_MFMA answer LBDRN_E_UNSUPPORTED, and no byte of the guarded parameters,
    moments, losses or workspaces changes."""
    s = R.Shape(*WR.HEADLINE, nl, act)
    assert WR.plan(s, bc) is None
    L = _lib.lib()
    n, bs = WR.H * WR.W, WR.BS_ODD
    net = ops.make_net(s.F, bc, s.C, nl, 1 if act == "relu" else 0)
    arena = Arena(dev)
    rng = np.random.default_rng(bc)
    slots = []
    for k in range(2):
        img, _, perm = WR.fit_inputs(R.Shape(*WR.HEADLINE, 2, "sine"), bc, 0, k)
        p0 = rng.uniform(-0.05, 0.05, ops.param_count(net)).astype(np.float32)
        msb, _, mx = O.split_bits(img, WR.K)
        geom = ops.FeatureGeometry(s.C, WR.H, WR.W, WR.K, s.D, mx, s.featcfg(), dev)
        nbytes = L.lbdrn_train_workspace(ctypes.byref(geom.c), ctypes.byref(net), bs)
        assert nbytes == WR.generic_workspace_bytes(s, bc, bs) > 0
        slots.append(dict(geom=geom, img=arena.const(img), msb=arena.const(msb), perm=arena.const(perm), p=arena.const(p0),
                          m=arena.const(rng.standard_normal(len(p0)).astype(np.float32)),
                          v=arena.const(rng.random(len(p0)).astype(np.float32)),
                          losses=arena.const(np.full(2, 7.0, np.float32)), ws=arena.buf(nbytes, 0xA5)))
    s0 = slots[0]
    arr = lambda key, count: (ctypes.c_void_p * count)(*[x[key].ptr for x in slots[:count]])
    calls = [lambda: ops._call(L.lbdrn_train_prepare, s0["p"].t, ctypes.byref(s0["geom"].c), ctypes.byref(net), s0["img"].ptr, s0["msb"].ptr,
                               bs, s0["ws"].ptr, s0["ws"].nbytes, MFMA),
             lambda: ops._call(L.lbdrn_train_epoch, s0["p"].t, ctypes.byref(s0["geom"].c), ctypes.byref(net), s0["img"].ptr, s0["msb"].ptr,
                               s0["perm"].ptr, n, bs, s0["p"].ptr, s0["m"].ptr, s0["v"].ptr, 0, LR, s0["losses"].ptr, s0["ws"].ptr,
                               s0["ws"].nbytes, MFMA)]
    for count in (1, 2):
        garr = (ctypes.POINTER(_lib.Geom) * count)(*[ctypes.pointer(x["geom"].c) for x in slots[:count]])
        calls.append(lambda count=count, garr=garr: ops._call(
            L.lbdrn_train_epoch_group, s0["p"].t, count, ctypes.cast(garr, ctypes.c_void_p), ctypes.byref(net), arr("img", count),
            arr("msb", count), arr("perm", count), n, bs, arr("p", count), arr("m", count), arr("v", count), 0, LR,
            arr("losses", count), arr("ws", count), s0["ws"].nbytes, MFMA))
    for k, call in enumerate(calls):
        with pytest.raises(_lib.LbdrnError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED, (k, e.value)
        torch.cuda.synchronize(dev)
        arena.check()
        for x in slots:
            assert bool((x["ws"].as_u8() == 0xA5).all()), k
