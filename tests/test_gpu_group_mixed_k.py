"""lbdrn_train_epoch_group and codec.fit_group / fit_many over the K points of ONE raster.

Every point of a K sweep re-seeds its generator (ref encode.py:200-205): for one image the points share the raster, F, n,
the initial weights and the permutations, and differ in the MSB plane, msb_max, the row matrix and the labels -- all of
which the group call takes per fit.  K is read by the row build of lbdrn_train_prepare only (include/lbdrn_hip.h), so a
group of fits whose K differs steps exactly as the single calls do.  Every comparison here is bit identity; no tolerance.

  * the group call against one lbdrn_train_epoch per fit: groups of 2, 3 and 4 fits of one 16 x 24 raster of 16-bit
    samples at K = (2, 6), (1, 4, 7), (3, 5, 6, 8) -- msb_max = max >> K differs between the fits by construction --, two
    epochs of minibatches of 100 rows (three full ones and a short last one of 84), once with ONE permutation tensor
    handed over for every fit and once with a tensor (and an order) per fit; at the smallest shape of every stepping
    path: 8 bands D 2 nl 2 (LQ 48: streamed pairs), 4 bands (LQ 24), nl 1, ReLU, 6 bands D 3 (LQ 96: k_train_split steps
    the group), 4 bands nl 3 (the tile kernel, which has no 8-band D 2 instance: fit after fit inside the call) and
    bc 128 (likewise); on PATH_GENERIC, PATH_MFMA and PATH_AUTO;
  * refusals: a group that differs in H, in D or in C is LBDRN_E_ARG and no byte of the guarded state changes;
  * whole fits: codec.fit_group([img] * 3, K=[3, 5, 6]) and codec.fit_many with a K list and four in flight against three
    codec.fit_device calls (best_params, mse_log), 8 and 4 bands, three epochs;
  * a TrainWorkspace prepared at one K is refused with another K's geometry."""
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

import train_plan_reference as R  # noqa: E402
from guarded import Arena  # noqa: E402
from lbdrn_hip import _lib, codec, ops  # noqa: E402
from lbdrn_hip.features import FeatCfg  # noqa: E402

pytestmark = pytest.mark.gpu
GEN, MFMA, AUTO = _lib.PATH_GENERIC, _lib.PATH_MFMA, _lib.PATH_AUTO
H, W, BS, LR = 16, 24, 100, 1e-3
K_SETS = ((2, 6), (1, 4, 7), (3, 5, 6, 8))

# (id, bands, D, hidden layers, activation, bc, what steps a group of this shape)
SHAPES = (
    ("c8-d2-nl2", 8, 2, 2, "sine", 64, "stream"),
    ("c4-d2-nl2", 4, 2, 2, "sine", 64, "stream"),
    ("c8-d2-nl1", 8, 2, 1, "sine", 64, "stream"),
    ("c8-d2-nl2-relu", 8, 2, 2, "relu", 64, "stream"),
    ("c6-d3-nl2", 6, 3, 2, "sine", 64, "split"),
    ("c4-d2-nl3", 4, 2, 3, "sine", 64, "tile"),
    ("c8-d2-nl2-bc128", 8, 2, 2, "sine", 128, "wide"),
)


def _bits(a):
    return a.view(np.int32)


def _cfg(act):
    return FeatCfg(False, False, 1.4, 12, True, True, act)


def _init_params(rng, F, bc, C, nl, act):
    """uniform weights at the reference's scales (LBDRNmodel.py), a ReLU net's ten times larger (train_plan_reference)"""
    gain = 10.0 if act == "relu" else 1.0
    parts = []
    for layer in range(nl):
        nin = F if layer == 0 else bc
        b = (1.0 / nin if layer == 0 else np.sqrt(6.0 / nin) / 30.0) * gain
        parts += [rng.uniform(-b, b, bc * nin), rng.uniform(-b, b, bc)]
    b = np.sqrt(6.0 / bc) / 30.0 * gain
    parts += [rng.uniform(-b, b, C * bc), rng.uniform(-b, b, C)]
    return np.concatenate(parts).astype(np.float32)


class Sweep:
    """One raster, one set of initial weights and the fits of it at K = 1 .. 8: geometry, MSB plane and a workspace each."""

    def __init__(self, dev, C, D, nl, act, bc, path):
        rng = np.random.default_rng([C, D, nl, bc, len(act)])
        img = rng.integers(0, 1 << 16, (C, H, W)).astype(np.uint16)
        img[0, 0, 0] = 0xFFFF                                            # (msb_max = 0xFFFF >> K: differs for every K)
        self.dev, self.path, self.C, self.bc = dev, path, C, bc
        self.img_d = ops.to_device_u16(img, dev)
        cfg = _cfg(act)
        F = cfg.feature_dim(C, D)
        self.net = ops.make_net(F, bc, C, nl, cfg.act)
        self.p0 = _init_params(rng, F, bc, C, nl, act)
        assert len(self.p0) == ops.param_count(self.net)
        # one order for every K (the sweep's case) and one per K
        self.shared_perm = torch.from_numpy(rng.permutation(H * W).astype(np.int64)).to(dev)
        self.own_perm = {K: torch.from_numpy(rng.permutation(H * W).astype(np.int64)).to(dev) for K in range(1, 9)}
        self.fits = {}
        for K in range(1, 9):
            msb_d, mx = ops.split_bits(self.img_d, K)
            assert mx == 0xFFFF >> K
            geom = ops.FeatureGeometry(C, H, W, K, D, mx, cfg, dev)
            ws = ops.TrainWorkspace(geom, self.net, BS, dev).prepare(self.img_d, msb_d, path)
            self.fits[K] = (geom, msb_d, ws)
        self.steps = (H * W + BS - 1) // BS

    def perm(self, K, shared):
        return self.shared_perm if shared else self.own_perm[K]

    def state(self):
        p = torch.from_numpy(self.p0.copy()).to(self.dev)
        return p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(self.steps, dtype=torch.float32, device=self.dev)

    def single(self, K, shared):
        """two lbdrn_train_epoch calls -> [params, exp_avg, exp_avg_sq, losses]"""
        geom, msb_d, ws = self.fits[K]
        p, m, v, losses = self.state()
        for e in range(2):
            ops.train_epoch(geom, self.net, self.img_d, msb_d, self.perm(K, shared), BS, p, m, v, e * self.steps, LR, losses,
                            self.path, ws)
        return [t.cpu().numpy() for t in (p, m, v, losses)]

    def group(self, Ks, shared):
        """two lbdrn_train_epoch_group calls over the fits at Ks -> {K: [params, exp_avg, exp_avg_sq, losses]}"""
        st = [self.state() for _ in Ks]
        perms = [self.perm(K, shared) for K in Ks]
        assert (len({t.data_ptr() for t in perms}) == 1) == shared
        for e in range(2):
            ops.train_epoch_group([self.fits[K][0] for K in Ks], self.net, [self.img_d] * len(Ks), [self.fits[K][1] for K in Ks],
                                  perms, BS, [s[0] for s in st], [s[1] for s in st], [s[2] for s in st], e * self.steps, LR,
                                  [s[3] for s in st], self.path, [self.fits[K][2] for K in Ks])
        return {K: [t.cpu().numpy() for t in s] for K, s in zip(Ks, st)}


@pytest.mark.parametrize("path", [pytest.param(GEN, id="generic"), pytest.param(MFMA, id="mfma"), pytest.param(AUTO, id="auto")])
@pytest.mark.parametrize("shape", [pytest.param(s, id=s[0]) for s in SHAPES])
def test_group_of_mixed_k_equals_the_single_calls(dev, shape, path):
    _, C, D, nl, act, bc, kind = shape
    if bc == 64:     # the shape steps where its line of SHAPES says (tests/train_plan_reference.py restates the launch plan)
        plan = R.Shape(0, 0, 1, 1, C, D, nl, act).plan()
        assert plan["kind"] == ("tile" if kind == "tile" else "stream") and R.takes_groups(plan) == (kind != "tile")
        if kind != "tile":
            assert (R.Shape(0, 0, 1, 1, C, D, nl, act).instance(count=2)[0] == "split") == (kind == "split")
    sw = Sweep(dev, C, D, nl, act, bc, path)
    assert ops.train_group_size(C, H, W, 3, D, _cfg(act), bc, nl) == (4 if kind in ("stream", "split") else 1)
    single = {(K, shared): sw.single(K, shared) for shared in (True, False) for K in sorted({k for ks in K_SETS for k in ks})}
    p, m, v, losses = single[(5, True)]
    assert np.isfinite(p).all() and np.isfinite(losses).all() and np.abs(m).max() > 0 and sw.steps == 4
    # the K points really are different fits: another MSB plane, other labels
    assert not np.array_equal(_bits(single[(2, True)][0]), _bits(single[(6, True)][0]))
    for Ks in K_SETS:
        for shared in (True, False):
            got = sw.group(Ks, shared)
            for K in Ks:
                for name, a, c in zip(("params", "exp_avg", "exp_avg_sq", "losses"), got[K], single[(K, shared)]):
                    assert np.array_equal(_bits(a), _bits(c)), (Ks, shared, K, name)


def _raw_group(slots, net, n, bs, path, ref):
    arr = lambda key: (ctypes.c_void_p * len(slots))(*[s[key].ptr for s in slots])
    garr = (ctypes.POINTER(_lib.Geom) * len(slots))(*[ctypes.pointer(s["geom"].c) for s in slots])
    ops._call(_lib.lib().lbdrn_train_epoch_group, ref, len(slots), ctypes.cast(garr, ctypes.c_void_p), ctypes.byref(net), arr("img"),
              arr("msb"), arr("perm"), n, bs, arr("p"), arr("m"), arr("v"), 0, LR, arr("losses"), arr("ws"), slots[0]["ws"].nbytes, path)


@pytest.mark.parametrize("differs", ["H", "D", "C"])
def test_a_group_of_two_shapes_is_still_refused_and_writes_nothing(dev, differs):
    """K left the list of what must agree; H (with it n's meaning), D and C did not.  The second fit's geometry differs in
    one of them -- its own buffers are sized for its own shape, so that nothing but the shape check can object -- and the
    call answers LBDRN_E_ARG with every guarded buffer as it was."""
    cfg = _cfg("sine")
    rng = np.random.default_rng(7)
    arena = Arena(dev)
    base = dict(C=8, H=H, W=W, D=2)
    other = dict(base, **{"H": {"H": H + 1}, "D": {"D": 1}, "C": {"C": 4}}[differs])
    net = ops.make_net(cfg.feature_dim(8, 2), 64, 8, 2, cfg.act)
    slots = []
    for K, s in ((3, base), (5, other)):
        img = rng.integers(0, 1 << 16, (s["C"], s["H"], s["W"])).astype(np.uint16)
        msb = img >> K
        geom = ops.FeatureGeometry(s["C"], s["H"], s["W"], K, s["D"], int(msb.max()), cfg, dev)
        own = ops.make_net(cfg.feature_dim(s["C"], s["D"]), 64, s["C"], 2, cfg.act)
        nbytes = max(_lib.lib().lbdrn_train_workspace(ctypes.byref(geom.c), ctypes.byref(own), BS),
                     _lib.lib().lbdrn_train_workspace(ctypes.byref(slots[0]["geom"].c if slots else geom.c), ctypes.byref(net), BS))
        assert nbytes > 0
        npar = max(ops.param_count(net), ops.param_count(own))
        slots.append(dict(geom=geom, img=arena.const(img), msb=arena.const(msb),
                          perm=arena.const(rng.permutation(H * W).astype(np.int64)),
                          p=arena.const(rng.standard_normal(npar).astype(np.float32) * 0.01),
                          m=arena.const(rng.standard_normal(npar).astype(np.float32)),
                          v=arena.const(rng.random(npar).astype(np.float32)),
                          losses=arena.const(np.full(4, 7.0, np.float32)), ws=arena.buf(nbytes, 0xA5)))
    for path in (MFMA, GEN):
        with pytest.raises(_lib.LbdrnError) as e:
            _raw_group(slots, net, H * W, BS, path, slots[0]["p"].t)
        assert e.value.code == _lib.E_ARG, (differs, path, e.value)
        torch.cuda.synchronize(dev)
        arena.check_guards()
        arena.check_consts()
        for s in slots:
            assert bool((s["ws"].as_u8() == 0xA5).all())


@pytest.mark.parametrize("C", [8, 4])
def test_whole_fits_at_a_k_list_equal_fit_device(dev, C):
    """codec.fit_group and codec.fit_many (four in flight: two pairs) over [img] * 3 at K = [3, 5, 6] with ONE FitDraws --
    best_params and mse_log of every K bit for bit those of codec.fit_device at that K with the same draws."""
    from lbdrn_hip.synth import synthetic_tile
    Ks, D, bc, nl, bs, epochs = [3, 5, 6], 2, 64, 2, 256, 3
    img_d = ops.to_device_u16(synthetic_tile(3, C, 40, 36), dev)
    cfg = FeatCfg()
    torch.manual_seed(19920517)
    draws = codec.draw_fit(cfg.feature_dim(C, D), bc, C, nl, epochs)
    p_before = draws.params.clone()
    want = []
    for K in Ks:
        fit = codec.fit_device(img_d, K, D, bc, nl, LR, bs, epochs, cfg=cfg, draws=draws, alone=False)
        want.append((fit.best_params.cpu().numpy(), fit.mse_log.cpu().numpy(), fit.msb_max))
    assert len({w[2] for w in want}) == 3
    grouped = codec.fit_group([img_d] * 3, Ks, D, bc, nl, LR, bs, epochs, cfg=cfg, draws=[draws] * 3)
    many = codec.fit_many([img_d] * 3, Ks, D, bc, nl, LR, bs, epochs, cfg=cfg, draws=[draws] * 3, in_flight=4)
    torch.cuda.synchronize(dev)
    for name, fits in (("fit_group", grouped), ("fit_many", many)):
        for K, fit, (bp, log, mx) in zip(Ks, fits, want):
            assert fit.msb_max == mx and int(fit.geom.c.K) == K, (name, K)
            assert np.array_equal(_bits(fit.best_params.cpu().numpy()), _bits(bp)), (name, K)
            assert np.array_equal(_bits(fit.mse_log.cpu().numpy()), _bits(log)), (name, K)
    assert torch.equal(draws.params, p_before)                       # the shared draws were only read
    with pytest.raises(ValueError):
        codec.fit_group([img_d] * 3, [3, 5], D, bc, nl, LR, bs, epochs, cfg=cfg, draws=[draws] * 3)


def test_a_workspace_prepared_at_one_k_is_refused_at_another(dev):
    sw = Sweep(dev, 8, 2, 2, "sine", 64, MFMA)
    (g3, msb3, ws3), (g5, msb5, ws5) = sw.fits[3], sw.fits[5]
    p, m, v, losses = sw.state()
    before = p.clone()
    with pytest.raises(_lib.LbdrnError, match="prepare"):
        ops.train_epoch(g5, sw.net, sw.img_d, msb5, sw.shared_perm, BS, p, m, v, 0, LR, losses, MFMA, ws3)
    with pytest.raises(_lib.LbdrnError, match="prepared for its image"):
        ops.train_epoch_group([g3, g5], sw.net, [sw.img_d] * 2, [msb3, msb5], [sw.shared_perm] * 2, BS, [p, p.clone()],
                              [m, m.clone()], [v, v.clone()], 0, LR, None, MFMA, [ws3, ws3])
    assert torch.equal(p, before)
    ops.train_epoch(g5, sw.net, sw.img_d, msb5, sw.shared_perm, BS, p, m, v, 0, LR, losses, MFMA, ws5)     # its own: taken
    assert not torch.equal(p, before)
